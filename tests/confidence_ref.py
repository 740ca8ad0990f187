"""TEST INFRASTRUCTURE - the float64 restatement of the CTC confidence laws (confidence.py, csrc/ctc_confidence.hip), written from the
formulas and independent of the package: the frame law through the normalised distribution p = softmax(x) itself (not through the
shifted sums the implementation keeps), and the three aggregations."""
import math

import numpy as np

METHODS = ("max_prob", "entropy", "tsallis")
ALPHAS = (0.33, 0.5, 2.0)
AGGREGATIONS = ("mean", "min", "prod")
VS = (2, 5, 67, 800, 2051)              # 67: the 4-byte loads, 800: the 16-byte loads, 2051: the row is read twice
SCALES = (0.5, 3.0, 12.0)


def settings():
    """Every (method, alpha) the tests cover."""
    return [("max_prob", 0.33), ("entropy", 0.33)] + [("tsallis", a) for a in ALPHAS]


def frame_law(x, method, alpha):
    """One row of any float dtype -> its confidence as a Python float, in float64.  p = exp(x - lse(x)):
    max_prob (V max p - 1) / (V - 1); entropy 1 - H(p) / ln V; tsallis (sum p^a - V^(1-a)) / (1 - V^(1-a)); clamped to [0, 1];
    a NaN entry or no finite maximum gives 0."""
    x = np.asarray(x, np.float64)
    V = x.shape[0]
    if np.isnan(x).any() or not np.isfinite(x.max()):
        return 0.0
    keep = x[x > -np.inf]
    m = keep.max()
    lse = m + math.log(np.exp(keep - m).sum())
    logp = keep - lse
    p = np.exp(logp)
    if method == "max_prob":
        c = (V * p.max() - 1.0) / (V - 1.0)
    elif method == "entropy":
        pos = p > 0
        c = 1.0 + float((p[pos] * logp[pos]).sum()) / math.log(V)
    else:
        u = float(V) ** (1.0 - alpha)
        c = (float(np.exp(alpha * logp).sum()) - u) / (1.0 - u)
    return min(max(c, 0.0), 1.0)


def frame_conf(lp, lengths, method, alpha):
    """[B, T, V] -> float64 [B, T], 0 for t >= T_b."""
    B, T, _ = lp.shape
    out = np.zeros((B, T), np.float64)
    for b in range(B):
        for t in range(min(max(int(lengths[b]), 0), T)):
            out[b, t] = frame_law(lp[b, t], method, alpha)
    return out


def aggregate(values, aggregation):
    """The aggregation of a non-empty sequence in float64."""
    v = [float(x) for x in values]
    if aggregation == "mean":
        return math.fsum(v) / len(v)
    if aggregation == "min":
        return min(v)
    return float(np.prod(np.asarray(v, np.float64)))


def span_conf(conf, spans, lengths, aggregation):
    """conf [B, T], spans [B, L, 2] -> float64 [B, L]: spans clipped to [0, T_b), an empty one gives 0."""
    B, T = conf.shape
    out = np.zeros((B, spans.shape[1]), np.float64)
    for b in range(B):
        Tb = min(max(int(lengths[b]), 0), T)
        for j in range(spans.shape[1]):
            f, e = max(int(spans[b, j, 0]), 0), min(int(spans[b, j, 1]), Tb)
            if f < e:
                out[b, j] = aggregate(conf[b, f:e], aggregation)
    return out


def make_logits(seed, B, T, V, scale):
    """float32 [B, T, V]: log_softmax of scale x standard normal, from numpy's generator seeded with (seed, V, scale)."""
    rng = np.random.default_rng([seed, V, int(scale * 10)])
    x = (scale * rng.standard_normal((B, T, V))).astype(np.float64)
    x = x - x.max(-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)
