"""The contract of the prototype contrastive term (include/simt_hip.h) restated in numpy, parametrised by the arithmetic:
np.float32 -- every operation rounded on its own, every sum sequential in index order -- and np.float64; the inputs the tests share; and the
comparator the GPU tests hold the launches to.  Nothing here imports the code under test.

The value bar is 7.24's and 7.26's form:  max|gpu - f64| <= FACTOR * err32 + REL * max|f64|,  err32 the error of the sequential float32
restatement on the same stored inputs; FACTOR = 4 allows for the GPU's different summation order (fixed before the first run), REL is four
float32 units of the largest value; a bf16 seed additionally gets half a bf16 unit of the float64 value, element by element."""
import numpy as np

from _feat_dist_ref import half_ulp_bf16, windows
from _proto_ref import _seq_sum, to_bf16

FACTOR = 4.0
REL = 2.0 ** -22
TILE = 32                  # cells per tile of simt_proto_contrast (include/simt_hip.h)
MISTAKES = ("no_fhat", "over_M", "unseen_in_denominator", "temp_twice", "shifted", "sign", "invalid_row_grad")


def cell_labels_ref(label, h, w, C, min_ratio, n=None):
    """label int64 [B, H, W] -> (lab uint8 [B*h*w], the number of cells whose class has n[c] > 0; n None: every labelled cell).  lab = c iff
    float32(count_c) >= float32(min_ratio) * float32(pixels), one float32 multiply; the lowest such c; else 255."""
    label = np.asarray(label)
    B, H, W = label.shape
    r = np.float32(min_ratio)
    out = np.full((B, h, w), 255, dtype=np.uint8)
    for b in range(B):
        for i, (r0, r1) in enumerate(windows(H, h)):
            for j, (c0, c1) in enumerate(windows(W, w)):
                win = label[b, r0:r1, c0:c1]
                bar = np.float32(r * np.float32(win.size))
                cnt = np.bincount(win[(win >= 0) & (win < C)].astype(np.int64).ravel(), minlength=C)
                hit = np.nonzero(cnt.astype(np.float32) >= bar)[0]
                if len(hit):
                    out[b, i, j] = hit[0]
    lab = out.reshape(-1)
    ok = lab < C
    if n is not None:
        ok = ok & (np.asarray(n)[np.minimum(lab, C - 1)] > 0)
    return lab, int(ok.sum())


def contrast_ref(F, lab, eta, n, temp, lam, gscale, dt, mistake=None, junk=None):
    """F [M, D] holds exactly the values of the device buffer; lab [M] bytes; eta [C, D], n [C].  -> dict(d [M], seed [M, D] (unrounded), out
    [3], N, seen [C] bool, valid [M] bool, degenerate [M] bool), all float arrays in `dt`.  `mistake`: one of MISTAKES, planted; `junk`: the
    rows an unseen class's eta takes where a mistake reads them."""
    with np.errstate(all="ignore"):
        F, lab, n = np.asarray(F).astype(dt), np.asarray(lab).astype(np.int64), np.asarray(n)
        eta = np.asarray(eta).astype(dt)
        M, D = F.shape
        C = len(n)
        T = dt(np.float32(temp))
        lam_g = dt(np.float32(float(lam) * float(gscale)))
        ne = np.zeros(C, dtype=dt)
        for c in np.nonzero(n > 0)[0]:
            ne[c] = np.sqrt(_seq_sum((eta[c] * eta[c]).astype(dt), dt)).astype(dt)
        seen = (n > 0) & (ne > 0) & np.isfinite(ne)
        if seen.sum() < 2:
            seen = np.zeros(C, dtype=bool)
        valid = (lab < C) & seen[np.minimum(lab, C - 1)]
        N = int(valid.sum())
        d, seed = np.zeros(M, dtype=dt), np.zeros((M, D), dtype=dt)
        res = dict(d=d, seed=seed, out=np.zeros(3), N=N, seen=seen, valid=valid, degenerate=np.zeros(M, dtype=bool))
        if N == 0:
            return res
        used = seen.copy()
        if mistake == "unseen_in_denominator":
            used = np.ones(C, dtype=bool)
            eta = np.where(seen[:, None], eta, np.asarray(junk).astype(dt))
            for c in np.nonzero(~seen)[0]:
                ne[c] = np.sqrt(_seq_sum((eta[c] * eta[c]).astype(dt), dt)).astype(dt)
        cs = np.nonzero(used)[0]
        rows = np.nonzero(valid)[0]
        f = F[rows]
        nf = np.sqrt(_seq_sum((f * f).astype(dt), dt)).astype(dt)
        good = (nf > 0) & np.isfinite(nf)
        res["degenerate"][rows[~good]] = True
        dot = np.zeros((len(rows), len(cs)), dtype=dt)
        for k in range(D):          # index order
            dot = (dot + (f[:, k, None] * eta[cs, k][None, :]).astype(dt)).astype(dt)
        cosv = (dot / (nf[:, None] * ne[cs][None, :]).astype(dt)).astype(dt)
        s = (cosv / T).astype(dt)
        if mistake == "temp_twice":
            s = (s / T).astype(dt)
        mx = s.max(axis=1)
        e = np.exp((s - mx[:, None]).astype(dt)).astype(dt)
        lse = (mx + np.log(_seq_sum(e, dt)).astype(dt)).astype(dt)
        q = np.exp((s - lse[:, None]).astype(dt)).astype(dt)
        ypos = np.searchsorted(cs, lab[rows])
        onehot = np.zeros_like(q)
        onehot[np.arange(len(rows)), ypos] = 1
        loss = (lse - s[np.arange(len(rows)), ypos]).astype(dt)
        a = (q - onehot).astype(dt)
        phat = (eta[cs] / ne[cs][:, None]).astype(dt)
        fhat = (f / nf[:, None]).astype(dt)
        g = np.zeros((len(rows), D), dtype=dt)
        for j in range(len(cs)):
            g = (g + (a[:, j, None] * phat[j][None, :]).astype(dt)).astype(dt)
        w = _seq_sum((a * cosv).astype(dt), dt)
        if mistake != "no_fhat":
            g = (g - (w[:, None] * fhat).astype(dt)).astype(dt)
        k_ = dt(lam_g / dt(M if mistake == "over_M" else N))
        coef = (k_ / (T * nf).astype(dt)).astype(dt)
        sd = (coef[:, None] * g).astype(dt)
        if mistake == "sign":
            sd = -sd
        loss = np.where(good, loss, dt(0))
        sd = np.where(good[:, None], sd, dt(0))
        d[rows] = loss
        seed[rows] = sd
        if mistake == "shifted":
            seed[:] = np.roll(seed, 1, axis=0)
        if mistake == "invalid_row_grad":
            bad = np.nonzero(~valid)[0]
            seed[bad] = sd[0] if len(bad) else 0
        # the scalars: per workgroup binary32 sums (here: in cell order), then double in index order
        S = float(_seq_sum(d.astype(dt)[None, :], dt)[0]) if dt == np.float32 else float(d.sum())
        res["out"] = np.array([float(lam) * S / N, S / N, float(N)])
        return res


def make_case(M, D, C, bf16=False, seed=0, unseen=2, ignore=0.15, temp=0.1, lam=0.1, gscale=1.0, stray=True):
    """Positive (post-ReLU-like) features at noise 0.5 per channel around the positive prototype of a drawn class; `ignore` of the cells carry
    255; with `stray` two cells are labelled with an unseen class.  F holds the stored values (bf16-rounded when bf16) as float32 [M, D].
    `unseen` classes have n = 0 and a row of eta that is never to be read (NaN); `junk` is what a mistaken reader would find there."""
    rng = np.random.default_rng(2700 + seed)
    proto = np.abs(rng.standard_normal((C, D))) + 0.1
    gone = rng.choice(C, size=min(unseen, C - 2), replace=False) if unseen else np.zeros(0, dtype=np.int64)
    truth = rng.choice(np.setdiff1d(np.arange(C), gone), size=M)
    F =np.maximum(proto[truth] + 0.5 * rng.standard_normal((M, D)), 0.0).astype(np.float32) + np.float32(0.01)
    if bf16:
        F = to_bf16(F)
    n = rng.integers(1, 30, size=C).astype(np.int32)
    eta = (proto + 0.05 * rng.standard_normal((C, D))).astype(np.float32)
    junk = np.abs(rng.standard_normal((C, D))).astype(np.float32)
    lab = truth.astype(np.uint8)
    if unseen:
        n[gone] = 0
        eta[gone] = np.nan
    lab[rng.random(M) < ignore] = 255
    if stray and len(gone) and M >= 4:
        lab[rng.choice(M, size=2, replace=False)] = gone[0]
    return dict(F=F, lab=lab, eta=eta, n=n, C=C, D=D, M=M, bf16=bf16, temp=float(np.float32(temp)), lam=lam, gscale=gscale, junk=junk)


def refs(case, mistake=None, dt=np.float64):
    k = case
    return contrast_ref(k["F"], k["lab"], k["eta"], k["n"], k["temp"], k["lam"], k["gscale"], dt, mistake, k["junk"])


def bar(ref32, ref64):
    err32 = float(np.abs(np.asarray(ref32, dtype=np.float64) - ref64).max()) if np.size(ref64) else 0.0
    return FACTOR * err32 + REL * float(np.abs(ref64).max() if np.size(ref64) else 0.0), err32


def check_contrast(got, case, report=None, r64=None, r32=None):
    """got: dict(d [M], seed [M, D], out [3]) of the launches on the case's stored inputs, as float arrays.  AssertionError names the first
    quantity outside its bar.  -> dict of gpu_err / err32 ratios (printed when `report` is a string)."""
    r64 = refs(case, dt=np.float64) if r64 is None else r64
    r32 = refs(case, dt=np.float32) if r32 is None else r32
    valid, ratios = r64["valid"], {}
    gd, gs, go = (np.asarray(got[q], dtype=np.float64) for q in ("d", "seed", "out"))
    assert gd.shape == r64["d"].shape and gs.shape == r64["seed"].shape and go.shape == (3,), (gd.shape, gs.shape, go.shape)
    assert go[2] == r64["out"][2], f"N: {go[2]}, expected {r64['out'][2]}"
    assert not np.isnan(gd).any() and not np.isnan(gs).any() and not np.isnan(go).any(), "NaN among the outputs"
    zero = ~valid | r64["degenerate"]
    assert (gd[zero] == 0).all(), "a row that is not valid (or is degenerate) has a loss"
    z = gs[zero]
    assert (z == 0).all() and not np.signbit(z).any(), f"{int((z != 0).sum())} non-zero and {int(np.signbit(z).sum())} negative-zero seed elements in rows that must be +0"
    b, e32 = bar(r32["d"], r64["d"])
    err = float(np.abs(gd - r64["d"]).max())
    ratios["d"] = err / e32 if e32 else 0.0
    assert err <= b, f"d: error {err:.3e} beyond the bar {b:.3e} (err32 {e32:.3e})"
    b, e32 = bar(r32["seed"], r64["seed"])
    errs = np.abs(gs - r64["seed"])
    half = half_ulp_bf16(r64["seed"]) * (r64["seed"] != 0) if case["bf16"] else 0.0
    ratios["seed"] = float(np.maximum(errs - half, 0.0).max()) / e32 if e32 else 0.0          # (a bf16 seed: what the rounding of the store does not explain)
    room = b + half
    bad = errs > room
    assert not bad.any(), (f"seed: {int(bad.sum())} elements in {int(bad.any(axis=1).sum())} rows beyond the bar {b:.3e} (err32 {e32:.3e}), worst "
                           f"error {float(errs[bad].max()):.3e}")
    b, e32 = bar(r32["out"][:2], r64["out"][:2])
    err = float(np.abs(go[:2] - r64["out"][:2]).max())
    ratios["out"] = err / e32 if e32 else 0.0
    assert err <= b, f"out: error {err:.3e} beyond the bar {b:.3e} (err32 {e32:.3e}): {go} against {r64['out']}"
    if report is not None:
        print(f"proto_contrast {report}: gpu_err / err32  d {ratios['d']:.3f}  seed {ratios['seed']:.3f}  out {ratios['out']:.3f}  N {r64['N']} of {len(valid)}")
    return ratios


def as_got(r, case):
    """A contrast_ref result in the shape check_contrast takes (the float32 restatement standing in for the device)."""
    seed = r["seed"].astype(np.float32)
    return dict(d=r["d"].astype(np.float32), seed=to_bf16(seed) if case["bf16"] else seed, out=r["out"].astype(np.float32))


# the shapes the CPU and GPU tests share, in 7.26's naming (M_D_C), and what each one is there for
CASES = {
    "bf16_70_2048_19": dict(M=70, D=2048, C=19, bf16=True),                      # the production row, tiles of 32 + 32 + 6
    "f32_243_1024_19": dict(M=243, D=1024, C=19, seed=1),
    "f32_9_8_2": dict(M=9, D=8, C=2, unseen=0, seed=2),                          # the minimum: half a k-step, one partial tile
    "f32_162_64_64": dict(M=162, D=64, C=64, seed=3),                            # two class tiles, every lane a class
    "bf16_363_128_19": dict(M=363, D=128, C=19, bf16=True, seed=4),              # twelve tiles
    "bf16_42_4096_5": dict(M=42, D=4096, C=5, bf16=True, unseen=1, seed=5),      # the widest row
    "f32_1_64_19": dict(M=1, D=64, C=19, seed=6, ignore=0.0, stray=False),       # tile edges
    "f32_31_64_19": dict(M=31, D=64, C=19, seed=7),
    "f32_32_64_19": dict(M=32, D=64, C=19, seed=8),
    "f32_33_64_19": dict(M=33, D=64, C=19, seed=9),
    "f32_40_24_19": dict(M=40, D=24, C=19, seed=10),                             # D % 16 == 8 and D % 32 == 24: the ragged k-step and channel block
}
_MADE = {}


def case(name):
    """make_case(**CASES[name]), made once and shared (read-only)."""
    if name not in _MADE:
        _MADE[name] = make_case(**CASES[name])
    return _MADE[name]
