"""Direction triples at the thresholds of the segment's reciprocal guard (rt_core.h recip_box_ok3,
seg_box_inv) and the reciprocals the parity contract asks for: RN(1 / x) clamped to +-2^100, a NaN
reciprocal to -2^100 (box_inv_clamp's maxNum, then minNum). The same values, in the same order,
as tests/c/guard_root_check.cpp's."""
import numpy as np

F = np.float32


def values():
    up = lambda x: np.nextafter(F(x), F(np.inf))  # noqa: E731
    down = lambda x: np.nextafter(F(x), F(-np.inf))  # noqa: E731
    mags = [F(0.0), F(2.0 ** -140), F(2.0 ** -101), down(2.0 ** -100), F(2.0 ** -100), up(2.0 ** -100), F(1.0),
            F(2.0 ** 125), down(2.0 ** 126), F(2.0 ** 126), up(2.0 ** 126), np.finfo(F).max, F(np.inf)]
    v = []
    for m in mags:
        v += [m, -m]
    bits = np.array(v, F).view(np.uint32).tolist() + [0x7FC00000, 0xFFC00001]  # NaN, a negative NaN with a payload
    return np.array(bits, np.uint32).view(F)


def triples():
    """[n, 3] f32: every triple of values(), x slowest."""
    v = values()
    x, y, z = np.meshgrid(v, v, v, indexing="ij")
    return np.ascontiguousarray(np.stack([x.ravel(), y.ravel(), z.ravel()], -1))


def clamped_recip(d):
    c = F(2.0 ** 100)
    with np.errstate(all="ignore"):
        inv = (F(1.0) / np.asarray(d, F)).astype(F)
        return np.fmin(np.fmax(inv, -c), c).astype(F)
