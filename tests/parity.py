"""shared parity helpers.  Tolerance = BASELINE.json north_star: logits within 1e-3 relative fp32
(max|d| <= 1e-3 * max|ref| and element-wise |d| <= 1e-3*|ref| + 1e-3*rms(ref)),
greedy ids identical wherever the reference's own top-2 margin exceeds that band.  TOL / _close: the tighter bound of the suites that check one
launch (tests/test_kernels_gpu.py) or one layer (tests/test_chunk_layers_gpu.py) against the oracle's piece for it."""
import numpy as np

REL = 1e-3
TOL = 3e-5          # relative to the vector's max |.|: an f32 GEMV of <= 20480 terms is good to ~1e-6, a wrong row or scale is O(1)


def _close(got, ref, what, tol=TOL):
    """one kernel's (or one layer's) output vector against its reference, relative to the reference's max |.|; returns the error"""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    assert np.isfinite(got).all(), what
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = float(np.abs(got - ref).max()) / scale
    assert err <= tol, f"{what}: max |d| / max |ref| = {err:.3e} > {tol:.0e}"
    return err


def check_logits(got, ref, what=""):
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite logits"
    d = np.abs(got - ref)
    mx = np.abs(ref).max(); rms = np.sqrt((ref ** 2).mean())
    assert d.max() <= REL * mx, f"{what}: max|d|={d.max():.3e} > {REL}*max|ref|={REL * mx:.3e}"
    bad = d > REL * np.abs(ref) + REL * rms
    assert not bad.any(), f"{what}: {bad.sum()} elements outside 1e-3*|ref| + 1e-3*rms"
    return d.max() / mx


def argmax_ban0(logits):
    l = np.array(logits, np.float32, copy=True); l[0] = -np.inf
    return int(np.argmax(l))


def check_argmax(got, ref, what=""):
    """identical greedy id, unless the reference's top-2 margin is inside the tolerance band"""
    g, r = argmax_ban0(got), argmax_ban0(ref)
    if g != r:
        rr = np.array(ref, np.float64); rr[0] = -np.inf
        top2 = np.sort(rr)[-2:]
        margin = top2[1] - top2[0]
        assert margin <= 2 * REL * np.abs(rr[np.isfinite(rr)]).max(), f"{what}: argmax {g} != {r} with margin {margin:.3e}"
    return g == r
