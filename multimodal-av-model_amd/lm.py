"""Token n-gram language model for shallow fusion in CTC prefix beam search (beam_search.prefix_beam_search(lm=...), csrc/ngram_lm.h, csrc/ctc_beam.hip).

``NGramLM`` is a backoff n-gram model over TOKEN IDS - the tokenizer's pieces, not words - of order 1 <= N <= 4 over a vocabulary of
V <= 65533 ids.  Every n-gram stores ``logp`` and ``backoff``, natural log, float32.  An optional begin-of-sentence id ``bos = V`` is never
predicted; it is only ever the oldest context token of the empty prefix.  End of sentence is not modelled: ``</s>`` n-grams are dropped when
an ARPA file is read, so a hypothesis pays nothing for ending.  A token without a unigram scores ``unk_logp`` (the file's ``<unk>`` if it
has one, else -10 ln 10, pyctcdecode's default), so every score is finite.

The scoring law (one wording for this file, csrc/ngram_lm.h and DESIGN §0.0d).  s(c | ctx), for m from min(N - 1, tokens available)
down to 1: look up the (m + 1)-gram "last m context tokens, c"; found: return acc + logp.  Not found: acc += backoff(the m-gram that is
the context), then drop the context's oldest token; a context that is absent adds nothing.  At m = 0 return acc + unigram(c).  acc starts
at 0; the additions are float32, in that order, and there is nothing else - no multiply, no libm - so the host and the device give the same
bits.

Keys are exact (no hash collisions to reason about): tokens w1..wn are packed oldest first as id + 1 in 16-bit fields, the newest in the
low field.  A prefix's context ``ctx`` is its last N - 1 tokens in the same packing, ctx' = ((ctx << 16) | (c + 1)) & mask(N - 1); the
empty prefix has ctx = bos + 1, or 0 without bos; a zero field means "context shorter than this order".

Device tables (``to_device``): ``unigrams`` float32 [V + 1][2] = (logp, backoff), row V = bos; and the n-grams of order >= 2 in an
open-addressing hash table of 16-byte slots {u64 key, f32 logp, f32 backoff}: power-of-two size, load <= 0.5, key 0 = empty, linear
probing from splitmix64(key) & (slots - 1); the longest probe run of a stored key is recorded and bounds every lookup."""
from __future__ import annotations

import math
import os
from collections import defaultdict

import numpy as np

LN10 = math.log(10.0)
DEFAULT_UNK_LOGP = -10.0 * LN10
MAX_ORDER = 4
MAX_VOCAB = 65533
_M64 = (1 << 64) - 1


def splitmix64(key: int) -> int:
    z = (key + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def pack_key(ids) -> int:
    """Tokens oldest first -> id + 1 in 16-bit fields, the newest in the low field."""
    k = 0
    for i in ids:
        k = (k << 16) | (int(i) + 1)
    return k


def unpack_key(key: int):
    out = []
    while key:
        out.append((key & 0xFFFF) - 1)
        key >>= 16
    return tuple(reversed(out))


def estimate_interpolated(sequences, vocab_size, blank, order=3, discount=0.75, bos=True):
    """Interpolated absolute discounting in backoff form, float64: {n-gram tuple: (P(w | h), bow(hw))} for every n-gram of the corpus, bos
    (= vocab_size) as the oldest token of a sentence's first n-grams.  bow(h) = D types(h) / c(h); a seen n-gram holds
    (c(hw) - D) / c(h) + bow(h) P(w | h'); unigrams are add-one over the non-blank tokens.  There is no quotient of sums (Katz's
    (1 - sum seen P) / (1 - sum seen P_low) divides by zero once a context has seen every token): the sum over the non-blank tokens is
    1 for every context by construction."""
    V, N, D = int(vocab_size), int(order), float(discount)
    counts = [defaultdict(int) for _ in range(N + 1)]            # counts[n][n-gram]
    for seq in sequences:
        seq = [int(x) for x in seq]
        if any(not 0 <= x < V or x == blank for x in seq):
            raise ValueError(f"NGramLM.from_corpus: a sentence holds an id outside [0, {V}) or the blank {blank}")
        toks = ([V] if bos else []) + seq
        for i in range(1 if bos else 0, len(toks)):
            for n in range(1, N + 1):
                if i - n + 1 < 0:
                    break
                counts[n][tuple(toks[i - n + 1:i + 1])] += 1
    total = sum(counts[1].values())
    est = {(w,): ((counts[1].get((w,), 0) + 1.0) / (total + V - 1.0), 1.0) for w in range(V) if w != blank}
    if bos:
        est[(V,)] = (0.0, 1.0)
    for n in range(2, N + 1):
        c_h, types = defaultdict(int), defaultdict(int)
        for g, c in counts[n].items():
            c_h[g[:-1]] += c
            types[g[:-1]] += 1
        for h, ch in c_h.items():
            p, _ = est[h]
            est[h] = (p, D * types[h] / ch)
        for g, c in counts[n].items():
            h = g[:-1]
            est[g] = ((c - D) / c_h[h] + est[h][1] * est[g[1:]][0], 1.0)
    return est


class DeviceLM:
    """The tables of one NGramLM on one device (NGramLM.to_device)."""

    def __init__(self, unigrams, table, slots, order, vocab_size, bos, probe_bound):
        self.unigrams, self.table, self.slots, self.order = unigrams, table, int(slots), int(order)
        self.vocab_size, self.bos, self.probe_bound = int(vocab_size), int(bos), int(probe_bound)


class NGramLM:
    def __init__(self, order, vocab_size, blank, unigrams, ngrams, bos=True, unk_logp=DEFAULT_UNK_LOGP):
        """unigrams: {id: (logp, backoff)} (id = vocab_size: bos, only its backoff is used); ngrams: {tuple of 2..order ids: (logp, backoff)};
        natural log.  Values are stored as float32."""
        self.order, self.vocab_size, self.blank, self.bos = int(order), int(vocab_size), int(blank), bool(bos)
        V = self.vocab_size
        if not 1 <= self.order <= MAX_ORDER:
            raise ValueError(f"NGramLM: order {self.order} outside [1, {MAX_ORDER}]")
        if not 2 <= V <= MAX_VOCAB or not 0 <= self.blank < V:
            raise ValueError(f"NGramLM: need 2 <= vocab_size <= {MAX_VOCAB} and 0 <= blank < vocab_size, got {V}, {self.blank}")
        self.unk_logp = np.float32(unk_logp)
        self.uni = np.zeros((V + 1, 2), np.float32)
        self.uni[:, 0] = self.unk_logp
        self.uni_present = np.zeros(V + 1, bool)
        for w, (lp, bo) in unigrams.items():
            if not 0 <= w <= V or (w == V and not self.bos):
                raise ValueError(f"NGramLM: unigram id {w} outside the vocabulary")
            self.uni[w] = (lp, bo)
            self.uni_present[w] = True
        self.uni_present[V] = self.bos
        self.table = {}
        for g, (lp, bo) in ngrams.items():
            g = tuple(int(x) for x in g)
            if not 2 <= len(g) <= self.order:
                raise ValueError(f"NGramLM: n-gram {g} has a length outside [2, order {self.order}]")
            if not all(0 <= x < V for x in g[1:]) or not (0 <= g[0] < V or (g[0] == V and self.bos)):
                raise ValueError(f"NGramLM: n-gram {g} holds an id outside the vocabulary (bos only as the oldest token)")
            self.table[pack_key(g)] = (np.float32(lp), np.float32(bo))
        if not np.isfinite(self.uni).all() or not all(np.isfinite(a) and np.isfinite(b) for a, b in self.table.values()):
            raise ValueError("NGramLM: every logp and backoff must be finite")
        self._devices = {}

    # ---- construction ----
    @classmethod
    def from_corpus(cls, sequences, vocab_size, blank, order=3, discount=0.75, bos=True):
        if not 0.0 < discount < 1.0:
            raise ValueError(f"NGramLM.from_corpus: discount {discount} outside (0, 1)")
        if not 1 <= int(order) <= MAX_ORDER:
            raise ValueError(f"NGramLM: order {order} outside [1, {MAX_ORDER}]")
        est = estimate_interpolated(sequences, vocab_size, blank, order, discount, bos)
        ln = lambda p, b: (math.log(p) if p > 0.0 else 0.0, math.log(b))
        uni = {g[0]: ln(*v) for g, v in est.items() if len(g) == 1}
        return cls(order, vocab_size, blank, uni, {g: ln(*v) for g, v in est.items() if len(g) > 1}, bos=bos)

    @classmethod
    def from_arpa(cls, text_or_path, token_to_id, vocab_size=None, blank=0):
        """A plain ARPA file (log10 in the file, ln in memory).  token_to_id: mapping (or callable) from the file's tokens to ids; ``<s>`` is
        bos, ``<unk>`` gives unk_logp, n-grams holding ``</s>`` are dropped (end of sentence is not modelled), and so are n-grams of order
        >= 2 holding ``<unk>`` or ``<s>`` anywhere but first.  The three names are ARPA's own: a vocabulary piece that is spelled like one of
        them (the tokenizer's ids 0, 1 and 2) cannot be named in a file - it is read as the special, never looked up in token_to_id - and
        to_arpa refuses to write it."""
        text = text_or_path
        if not (isinstance(text, str) and "\\data\\" in text):
            with open(os.fspath(text_or_path), encoding="utf-8") as f:
                text = f.read()
        look = token_to_id if callable(token_to_id) else token_to_id.__getitem__
        uni, grams, unk, bos, n, order = {}, {}, DEFAULT_UNK_LOGP, False, 0, 0
        rows = []
        for line in text.splitlines():
            line = line.strip()
            if not line or line == "\\data\\" or line.startswith("ngram "):
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                n = int(line[1:-7])
                order = max(order, n)
                continue
            parts = line.split()
            if n == 0 or len(parts) not in (n + 1, n + 2):
                raise ValueError(f"NGramLM.from_arpa: cannot read line {line!r}")
            rows.append((n, float(parts[0]) * LN10, parts[1:n + 1], float(parts[n + 1]) * LN10 if len(parts) == n + 2 else 0.0))
        if order == 0:
            raise ValueError("NGramLM.from_arpa: no n-gram section")
        bos = any(n == 1 and w[0] == "<s>" for n, _, w, _ in rows)
        ids_seen = []
        for n, lp, words, bo in rows:
            if "</s>" in words:
                continue
            if n == 1 and words[0] == "<unk>":
                unk = lp
                continue
            if n == 1 and words[0] == "<s>":
                uni[-1] = (0.0, bo)
                continue
            if "<unk>" in words or "<s>" in words[1:]:
                continue
            try:
                ids = [-1 if w == "<s>" else int(look(w)) for w in words]
            except (KeyError, IndexError) as e:
                raise ValueError(f"NGramLM.from_arpa: token {e} of the file is not in the vocabulary") from None
            ids_seen += ids
            (uni if n == 1 else grams)[ids[0] if n == 1 else tuple(ids)] = (lp, bo)
        V = int(vocab_size) if vocab_size is not None else max(ids_seen, default=0) + 1
        fix = lambda i: V if i == -1 else i
        return cls(order, V, blank, {fix(w): v for w, v in uni.items()}, {tuple(fix(i) for i in g): v for g, v in grams.items()},
                   bos=bos, unk_logp=unk)

    def to_arpa(self, id_to_token=None) -> str:
        """The model as ARPA text (log10, 17 significant digits: reading it back gives the same float32 values).  Tokens are written with
        id_to_token (mapping or callable), by default as their decimal id.  ``<s>``, ``</s>`` and ``<unk>`` are reserved by the format (from_arpa
        reads them as bos, end of sentence and the unknown token): a model that holds a token with one of these names - a transcript
        with the tokenizer's unk piece in it, say - would not read back as it was written, so that is a ValueError, not a silent loss.  The
        one exception: the bare unigram of such a token that no n-gram of order >= 2 holds (the add-one mass from_corpus gives a piece the
        transcripts never use) is left out of the file; read back, that token scores unk_logp."""
        name = (lambda i: str(i)) if id_to_token is None else (id_to_token if callable(id_to_token) else id_to_token.__getitem__)
        reserved = ("<s>", "</s>", "<unk>")

        def word(i):
            if i == self.vocab_size:
                return "<s>"
            w = str(name(i))
            if w in reserved or len(w.split()) != 1:
                raise ValueError(f"NGramLM.to_arpa: token {i} is named {w!r}, which an ARPA file cannot hold as a vocabulary token")
            return w
        by_n = {n: [] for n in range(1, self.order + 1)}
        by_n[1].append((float(self.unk_logp), ["<unk>"], 0.0))
        in_grams = {i for key in self.table for i in unpack_key(key)}
        for w in np.flatnonzero(self.uni_present):
            if w < self.vocab_size and w not in in_grams and str(name(int(w))) in reserved:
                continue                                                      # smoothing mass of a special piece no n-gram holds: left out
            by_n[1].append((-99.0 * LN10 if w == self.vocab_size else float(self.uni[w, 0]), [word(int(w))], float(self.uni[w, 1])))
        for key in sorted(self.table):
            g = unpack_key(key)
            by_n[len(g)].append((float(self.table[key][0]), [word(i) for i in g], float(self.table[key][1])))
        out = ["\\data\\"] + [f"ngram {n}={len(by_n[n])}" for n in by_n] + [""]
        for n, rows in by_n.items():
            out.append(f"\\{n}-grams:")
            for lp, words, bo in rows:
                tail = f"\t{bo / LN10!r}" if n < self.order and bo != 0.0 else ""
                out.append(f"{lp / LN10!r}\t{' '.join(words)}{tail}")
            out.append("")
        return "\n".join(out + ["\\end\\", ""])

    # ---- the law ----
    @property
    def ctx_mask(self) -> int:
        return (1 << (16 * (self.order - 1))) - 1

    @property
    def start_ctx(self) -> int:
        """Packed context of the empty prefix."""
        return (self.vocab_size + 1) & self.ctx_mask if self.bos else 0

    def push(self, ctx: int, c: int) -> int:
        return ((ctx << 16) | (int(c) + 1)) & self.ctx_mask

    def context(self, ids) -> int:
        ctx = self.start_ctx
        for c in ids:
            ctx = self.push(ctx, c)
        return ctx

    def score_ctx(self, ctx: int, c: int) -> np.float32:
        """s(c | ctx) on a packed context: the law of the module docstring, float32."""
        c = int(c)
        if not 0 <= c < self.vocab_size:
            raise ValueError(f"NGramLM.score: token {c} outside [0, {self.vocab_size})")
        acc = np.float32(0.0)
        m = self.order - 1
        while m >= 1 and (ctx >> (16 * (m - 1))) & 0xFFFF == 0:
            m -= 1
        while m >= 1:
            cm = ctx & ((1 << (16 * m)) - 1)
            e = self.table.get((cm << 16) | (c + 1))
            if e is not None:
                return acc + e[0]
            if m == 1:
                if cm - 1 <= self.vocab_size:
                    acc = acc + self.uni[cm - 1, 1]
            else:
                e = self.table.get(cm)
                if e is not None:
                    acc = acc + e[1]
            m -= 1
        return acc + self.uni[c, 0]

    def score(self, context_ids, token) -> np.float32:
        """s(token | context_ids): context_ids are all the tokens before it, oldest first (the last N - 1 count; bos stands before them)."""
        return self.score_ctx(self.context(context_ids), token)

    # ---- device tables ----
    def host_tables(self, slots=None):
        """(unigrams float32 [V + 1][2], table int64 [slots][2] = the 16-byte slots, slots, probe bound)."""
        n = len(self.table)
        need = 2
        while need < 2 * n:
            need *= 2
        slots = need if slots is None else int(slots)
        if slots < need or slots & (slots - 1):
            raise ValueError(f"NGramLM.to_device: slots {slots} must be a power of two >= {need} (load <= 0.5)")
        tab = np.zeros(slots, dtype=[("key", "<u8"), ("logp", "<f4"), ("backoff", "<f4")])
        keys = tab["key"]
        bound = 1
        for key, (lp, bo) in self.table.items():
            i, run = splitmix64(key) & (slots - 1), 1
            while keys[i] != 0:
                i, run = (i + 1) & (slots - 1), run + 1
            tab[i] = (key, lp, bo)
            bound = max(bound, run)
        return self.uni.copy(), tab.view("<i8").reshape(slots, 2), slots, bound

    def to_device(self, device, slots=None) -> DeviceLM:
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:                   # "cuda" and "cuda:0" are one device: one copy of the table
            device = torch.device("cuda", torch.cuda.current_device())
        hit = self._devices.get((str(device), slots))
        if hit is None:
            uni, tab, slots_, bound = self.host_tables(slots)
            hit = DeviceLM(torch.from_numpy(uni).to(device), torch.from_numpy(tab).to(device), slots_, self.order, self.vocab_size,
                           self.vocab_size if self.bos else -1, bound)
            self._devices[(str(device), slots)] = hit
        return hit

    def score_batch(self, ids, lens=None):
        """ids int32 [B][Lmax] on the GPU (lens [B], default Lmax) -> float32 [B][Lmax], out[b][i] = s(ids[b][i] | ids[b][:i]) for
        i < lens[b] and 0 after: av_ngram_score, one thread per token.  For n-best rescoring and perplexity."""
        import torch
        from . import _lib as L
        from . import ops
        if not ids.is_cuda or ids.dim() != 2:
            raise ValueError("NGramLM.score_batch: ids must be a [B, Lmax] tensor on the GPU")
        ids = ids.to(torch.int32).contiguous()
        B, Lmax = ids.shape
        ln = None if lens is None else torch.as_tensor(lens).to(device=ids.device, dtype=torch.long).contiguous()
        d = self.to_device(ids.device)
        out = torch.empty((B, Lmax), dtype=torch.float32, device=ids.device)
        L.check(L.lib().av_ngram_score(ops.ptr(ids), ops.ptr(ln), ops.ptr(out), B, Lmax, ops.ptr(d.unigrams), ops.ptr(d.table), d.slots, d.order,
                                       d.vocab_size, d.bos, d.probe_bound, ops.stream()), "av_ngram_score")
        return out
