"""CPU: the row law of csrc/ctc_common.h - "the strides cover [B][T][V] rows" - is one law in every CTC entry point that takes a strided
block of log-probs, in both libraries: the same rejected stride pairs give a status and a message that names the entry point and the
strides.  Argument errors only: nothing is launched."""
from conftest import pkg

B, T, V = 2, 4, 8
P = 4096                                         # any non-null address: argument checks come before a launch, nothing is dereferenced
BIG = 1 << 40                                    # workspace bytes: the strides are checked first

# (stride_b, stride_t) that cover neither [B][T][V] nor [T][B][V]
REJECTED = (
    (8, 8),                                      # both orders too short
    (31, 8),                                     # one short of T * stride_t
    (8, 15),                                     # one short of B * stride_b
    (7, 32),                                     # below V
    (-32, 8),                                    # negative
    (2 ** 62, 2 ** 62),                          # T * stride_t and B * stride_b overflow: only the quotient form rejects it for the right reason
)
# the long-form entry points take [S][rows][V] only: a block laid out rows first, which the others accept, is rejected too
REJECTED_ONE_ORDER = REJECTED + ((8, 16),)

# entry point -> its arguments around (stride_outer, stride_row); S_max = 5 (Lmax = 2), blank 0, N = 2 hypotheses
EITHER_ORDER = {
    "av_ctc_loss_fwd": lambda sb, st: (P, sb, st, P, 2, P, P, B, T, V, 5, 0, 1, P, None, None, None),
    "av_ctc_loss_bwd": lambda sb, st: (P, sb, st, P, 2, P, P, B, T, V, 5, 0, P, P, P, P, P, None),
    "av_ctc_nbest_fwd": lambda sb, st: (P, sb, st, P, 4, 2, P, P, B, 2, T, V, 5, 0, P, None, None, None),
    "av_ctc_nbest_bwd": lambda sb, st: (P, sb, st, P, 4, 2, P, P, B, 2, T, V, 5, 0, P, P, P, P, P, None),
    "av_ctc_align": lambda sb, st: (P, sb, st, P, 2, P, P, B, T, V, 5, 0, P, P, P, P, P, BIG, None),
    "av_ctc_frame_conf": lambda sb, st: (P, sb, st, None, B, T, V, 1, 0.0, P, None),
    "av_ctc_greedy_timed": lambda sb, st: (P, sb, st, None, B, T, V, 0, 1, 0.0, 0, P, P, P, P, P, None),
}
ONE_ORDER = {
    "av_ctc_stitch": lambda ss, sr: (P, ss, sr, P, P, B, T, T, V, P, None),                  # S = 2 speakers, R = 4 window rows, F = 4
    "av_ctc_cut_points": lambda ss, st: (P, ss, st, B, T, V, 0, 3, 0, P, None),              # segment 3, radius 0
    "av_ctc_segment_gather": lambda ss, st: (P, ss, st, P, B, T, V, 0, 3, P, P, None),       # nb 0, segment 3
}


def _libs():
    L = pkg("_lib"); Pm = pkg("precision")
    old = Pm.get_precision()
    out = []
    try:
        for mode, suffix in (("fp32", "libavhip.so"), ("fp16", "libavhip_f16.so")):
            Pm.set_precision(mode)
            lib = L.lib()
            assert lib._name.endswith(suffix)
            out.append(lib)
    finally:
        Pm.set_precision(old)
    return out


def test_every_entry_point_rejects_the_same_stride_pairs_by_name():
    for lib in _libs():
        for table, pairs in ((EITHER_ORDER, REJECTED), (ONE_ORDER, REJECTED_ONE_ORDER)):
            for name, args in table.items():
                for so, sr in pairs:
                    assert getattr(lib, name)(*args(so, sr)) != 0, (name, so, sr)
                    msg = lib.av_last_error()
                    assert b"strides" in msg and name.encode() in msg, (name, so, sr, msg)
