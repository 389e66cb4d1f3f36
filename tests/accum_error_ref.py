"""The error estimate of progressive accumulation (FR_FLAG_ACCUM_ERROR) restated in numpy f32:
fo-rma_amd/csrc/accum_error.h operation for operation, every one rounded once in f32
(tests/test_accum_error_host.py holds this against the header's own bits). Shared by the host
and the GPU tests; not a test module."""
import numpy as np

F = np.float32
FLOOR = F(2.0 ** -7)  # FR_ERR_FLOOR


def sq_term(s, spp):
    """What a frame of sum s and spp samples adds to Q: RN(RN(s * s) / (float)spp)."""
    s = np.asarray(s, F)
    with np.errstate(all="ignore"):
        return ((s * s).astype(F) / F(spp)).astype(F)


def variance(a, q, n, frames):
    """(m, v) per channel: m = A / fn, v = fmax((Q - RN(A * m)) / fk, 0), NaN -> 0."""
    a, q = np.asarray(a, F), np.asarray(q, F)
    fn, fk = F(n), F(frames - 1)
    with np.errstate(all="ignore"):
        m = (a / fn).astype(F)
        v = np.fmax(((q - (a * m).astype(F)).astype(F) / fk).astype(F), F(0))  # fmax: a NaN reads 0
    return m, v


def rel_error(a, q, n, frames):
    """rel [...] from A, Q [..., 3]: sqrt(((v_r + v_g) + v_b) / fn) over fmax((m_r + m_g) + m_b,
    2^-7); 0 where the summed mean is NaN or infinite."""
    m, v = variance(a, q, n, frames)
    fn = F(n)
    with np.errstate(all="ignore"):
        err = np.sqrt((((v[..., 0] + v[..., 1]).astype(F) + v[..., 2]).astype(F) / fn).astype(F)).astype(F)
        msum = ((m[..., 0] + m[..., 1]).astype(F) + m[..., 2]).astype(F)
        den = np.fmax(msum, FLOOR)
        rel = (err / den).astype(F)
    return np.where(np.isfinite(msum), rel, F(0)).astype(F)


class ErrorComposite:
    """The expected accumulators A and Q and what fr_ctx_accum_error reports, in numpy f32."""

    def __init__(self):
        self.a = self.q = None
        self.n = self.frames = 0

    def add(self, s, spp):
        """Adds a frame's per-pixel sum s [H, W, 3]; returns the mean A / n."""
        t = sq_term(s, spp)
        self.a = s.astype(F).copy() if self.a is None else (self.a + s).astype(F)
        self.q = t if self.q is None else (self.q + t).astype(F)
        self.n += spp
        self.frames += 1
        return (self.a / F(self.n)).astype(F)

    def rel(self):
        return rel_error(self.a, self.q, self.n, self.frames)

    def summary(self, threshold, rows=None):
        """{frames, samples, pixels, converged, max_rel} over the image, or over `rows` of it."""
        rel = self.rel() if rows is None else self.rel()[rows]
        return {"frames": self.frames, "samples": self.n, "pixels": int(rel.size),
                "converged": int(np.count_nonzero(rel <= F(threshold))), "max_rel": F(rel.max())}
