"""numpy restatement of the weight EMA's arithmetic contract (include/simt_hip.h, simt_ema_desc) -- the reference of
tests/test_ema_cpu.py and tests/test_gpu_ema.py.  The kernel is never compared with itself.

numpy rounds every float32 operation on its own (no FMA, gradual underflow), which is exactly what the contract asks of the kernel:
    omd == 1:   e = w                 as 32-bit words (NaN payloads and -0.0 survive)
    otherwise:  t = w - e;  u = omd * t;  e = e + u      (three IEEE binary32 roundings)
"""
import numpy as np


def omd(decay, t):
    """1 - decay of the update with 0-based index t: float32(max(1 - D, 1 / (t + 1))), computed in float64, rounded once."""
    return np.float32(max(1.0 - float(decay), 1.0 / (float(int(t)) + 1.0)))


def update(e, w, omd_t):
    """One update of the float32 array e towards w; returns the new e (inputs are not modified)."""
    e, w, omd_t = np.ascontiguousarray(e), np.ascontiguousarray(w), np.float32(omd_t)
    assert e.dtype == np.float32 and w.dtype == np.float32 and e.shape == w.shape
    assert np.float32(0) < omd_t <= np.float32(1)
    if omd_t == np.float32(1):
        return w.view(np.uint32).copy().view(np.float32)
    with np.errstate(all="ignore"):
        t = (w - e).astype(np.float32)
        u = (omd_t * t).astype(np.float32)
        return (e + u).astype(np.float32)


class Shadow:
    """The host twin of simt_amd.ema.WeightEma: {name: float32 array}, initialised as a copy, update(masters) with the schedule."""

    def __init__(self, masters, decay):
        self.decay, self.updates = float(decay), 0
        self.e = {k: np.array(v, dtype=np.float32, copy=True) for k, v in masters.items()}

    def update(self, masters):
        o = omd(self.decay, self.updates)
        for k in self.e:
            self.e[k] = update(self.e[k], np.asarray(masters[k], dtype=np.float32), o)
        self.updates += 1


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def planted(n, rng):
    """(w, e): random normals with the special values of the contract planted at fixed positions (where n allows): +-0, denormals, +-inf,
    pairs whose difference underflows, NaNs with payloads (in w only, in e only, in both)."""
    w = rng.standard_normal(n).astype(np.float32)
    e = rng.standard_normal(n).astype(np.float32)
    tiny = np.float32(1.1754944e-38)                        # FLT_MIN
    den = np.float32(1e-41)
    nan_a = np.array([0x7FC12345], dtype=np.uint32).view(np.float32)[0]
    nan_b = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]          # sign set, another payload
    plant = [(0.0, 0.0), (-0.0, -0.0), (-0.0, 0.0), (0.0, -0.0), (den, 0.0), (0.0, den), (den, -den), (np.inf, 1.0), (1.0, -np.inf),
             (np.inf, np.inf), (-np.inf, np.inf), (tiny * np.float32(1.5), tiny), (tiny, tiny * np.float32(1.25)), (nan_a, 1.0), (2.0, nan_b),
             (nan_a, nan_b), (3.0, 3.0), (np.float32(3.4e38), np.float32(-3.4e38)), (den, den)]
    wb, eb = w.view(np.uint32), e.view(np.uint32)           # planted as words: no conversion may touch a NaN's payload
    for i, (a, b) in enumerate(plant):
        j = (7 * i + 1) % n if n > 160 else i               # spread over the array where it is long enough, packed at the front otherwise
        if i < n:
            wb[j], eb[j] = np.array([a], dtype=np.float32).view(np.uint32)[0], np.array([b], dtype=np.float32).view(np.uint32)[0]
    return w, e
