"""Independent numpy restatement of the augmentation laws for the tests: the counter-hash generator of csrc/av_common.h in
uint32 arithmetic, the lip law as explicit loops over (b, t, y, x), the noise law sample by sample in arrays.  Shares no code with the
package's host path (augment.py)."""
import numpy as np

S_LIP = {1: 0xF0000011, 2: 0xF0000012}
S_SNR, S_NOISE = 0xF0000013, 0xF0000014
U32 = np.uint32
INV_STD = np.float32(1.0 / np.sqrt((65536.0 ** 2 - 1.0) / 3.0))


def _u32(v):
    return np.asarray(v, dtype=np.uint64).astype(U32)


def drop_key(seed, stream):
    with np.errstate(over="ignore"):
        seed = int(seed)
        h = _u32(seed & 0xFFFFFFFF) * U32(0x9E3779B1)
        h = h ^ (_u32(seed >> 32) * U32(0x85EBCA77))
        h = h ^ ((_u32(stream) + U32(0x165667B1)) * U32(0xC2B2AE3D))
        h = h ^ (h >> U32(15)); h = h * U32(0x2C1B3C6D); h = h ^ (h >> U32(12)); h = h * U32(0x297A2D39); h = h ^ (h >> U32(15))
    return h


def drop_key2(key):
    with np.errstate(over="ignore"):
        h = ((key << U32(16)) | (key >> U32(16))) * U32(0x9E3779B1) + U32(0x7F4A7C15)
        h = h ^ (h >> U32(13)); h = h * U32(0x5BD1E995); h = h ^ (h >> U32(15))
    return h


def mix32(x, k2):
    with np.errstate(over="ignore"):
        x = x ^ (x >> U32(16)); x = x * U32(0x7FEB352D); x = x ^ k2; x = x ^ (x >> U32(15)); x = x * U32(0x846CA68B); x = x ^ (x >> U32(16))
    return x


def drop_draw(seed, stream, block):
    """The two 32-bit words of block(s) ``block`` (drop_draw's idx4 >> 2), uint32 arrays of block's shape."""
    blk = np.asarray(block, dtype=np.uint64)
    c1 = (blk >> np.uint64(32)).astype(U32)
    key = drop_key(seed, stream); k2 = drop_key2(key)
    rot = lambda v, r: (v << U32(r)) | (v >> U32(32 - r))
    with np.errstate(over="ignore"):
        x = (blk & np.uint64(0xFFFFFFFF)).astype(U32) ^ key ^ c1 ^ rot(c1, 11) ^ rot(c1, 23)
        return mix32(x, k2), mix32(x + U32(0x9E3779B9), k2)


def uniforms16(seed, stream, block):
    """k0..k3 of one block as python ints."""
    o0, o1 = drop_draw(seed, stream, np.uint64(block))
    o0, o1 = int(o0), int(o1)
    return [o0 & 0xFFFF, o0 >> 16, o1 & 0xFFFF, o1 >> 16]


def draw(k, R):
    return (k * R) >> 16


def lip_plan(b, T, n, seed, step, speaker, S, flip_thr, Wmax, E):
    """(dx, dy, flip, tsrc list of T entries; -1 = padded) of clip b."""
    c = step * 65536 + b
    k = uniforms16(seed, S_LIP[speaker], c * 64)
    dx, dy, flip = draw(k[0], 2 * S + 1) - S, draw(k[1], 2 * S + 1) - S, k[2] < flip_thr
    spans = []
    nseg = (n + E - 1) // E
    for j in range(nseg):
        kk = uniforms16(seed, S_LIP[speaker], c * 64 + 1 + j // 2)
        s, w = draw(kk[2 * (j % 2)], E), draw(kk[2 * (j % 2) + 1], Wmax + 1)
        spans.append((j * E + s, min(j * E + s + w, n)))
    tsrc = []
    for t in range(T):
        if t >= n:
            tsrc.append(-1); continue
        j = t // E
        src = t
        if j > 0 and spans[j - 1][0] <= t < spans[j - 1][1]:
            src = max(spans[j - 1][0] - 1, 0)
        if spans[j][0] <= t < spans[j][1]:                         # the own segment's span wins
            src = max(spans[j][0] - 1, 0)
        tsrc.append(src)
    return dx, dy, flip, tsrc


def lips(x, lengths, seed, step, speaker, S, flip_thr, Wmax, E):
    """x float32 [B, T, H, W] -> the augmented clips, element by element."""
    B, T, H, W = x.shape
    out = np.zeros_like(x)
    for b in range(B):
        n = T if lengths is None else max(0, min(T, int(lengths[b])))
        dx, dy, flip, tsrc = lip_plan(b, T, n, seed, step, speaker, S, flip_thr, Wmax, E)
        for t in range(T):
            if tsrc[t] < 0:
                continue
            for y in range(H):
                ys = min(max(y - dy, 0), H - 1)
                for xx in range(W):
                    xf = W - 1 - xx if flip else xx
                    out[b, t, y, xx] = x[b, tsrc[t], ys, min(max(xf - dx, 0), W - 1)]
    return out


def noise_z(seed, step, b, n):
    """z_0 .. z_{n-1} of row b, float32."""
    c = step * 65536 + b
    o0, o1 = drop_draw(seed, S_NOISE, np.uint64(c << 24) + np.arange(n, dtype=np.uint64))
    s = (o0 & U32(0xFFFF)).astype(np.int64) + (o0 >> U32(16)).astype(np.int64) + (o1 & U32(0xFFFF)).astype(np.int64) + (o1 >> U32(16)).astype(np.int64)
    return (s - 131070).astype(np.float32) * INV_STD


def snr_db(seed, step, b, lo, hi):
    u = np.float32(uniforms16(seed, S_SNR, step * 65536 + b)[0]) / np.float32(65536.0)
    lo, hi = np.float32(lo), np.float32(hi)
    return np.float32(lo + np.float32(u * np.float32(hi - lo)))


def power(x, n):
    return float(np.sum(x[:n].astype(np.float64) ** 2) / n) if n > 0 else 0.0


def sigma64(x, n, seed, step, b, lo, hi):
    """The noise level of row b by the float64 law, before the rounding to float32."""
    return float(np.sqrt(power(x, n) * 10.0 ** (-float(snr_db(seed, step, b, lo, hi)) / 10.0)))


def noise(x, lengths, seed, step, lo, hi, sigma=None):
    """x float32 [B, N] -> (y, sigma float32 [B]); ``sigma``: use these levels (the device's) instead of the law's own."""
    B, N = x.shape
    y = x.copy()
    sg = np.zeros(B, np.float32)
    for b in range(B):
        n = max(0, min(N, int(lengths[b])))
        sg[b] = np.float32(sigma64(x[b], n, seed, step, b, lo, hi)) if sigma is None else np.float32(sigma[b])
        if n == 0 or sg[b] == 0:
            continue
        y[b, :n] = x[b, :n] + np.float32(sg[b] * noise_z(seed, step, b, n))
    return y, sg
