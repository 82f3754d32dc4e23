"""The contract of the prototype weights (include/simt_hip.h) restated in numpy, parametrised by the arithmetic: np.float32 --
every operation rounded on its own, every sum sequential in index order -- and np.float64; the inputs the tests share; and the comparator
the GPU tests hold the three launches to.  Nothing here imports the code under test.

The value bar is FDA's form (tests/_fda_ref.py):  max|gpu - f64| <= FACTOR * err32 + REL * max|f64|,  err32 the error of the sequential
float32 restatement on the same stored inputs; FACTOR allows for the GPU's different summation order, REL is four float32 units of the
largest value.  `lab` and the arg-max are discrete: a cell is EXCLUDED from them when the float64 top two of `out` lie within EXCL * bar of
each other or its `conf` within EXCL * bar of thr; the excluded share must stay below CAP (a condition on the inputs, not a budget)."""
import numpy as np

FACTOR = 4.0
REL = 2.0 ** -22
EXCL = 8.0
CAP = 0.01
PART_CELLS = 256           # cells per accumulate part (include/simt_hip.h)
MISTAKES = ("no_root", "unseen_at_zero", "unseen_weight_zero", "update_first", "momentum_swapped", "mean_over_cells", "no_renorm")


def to_bf16(x):
    """float32 values rounded to the nearest bf16 (ties to even), returned as float32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def first_argmax(v):
    """[M, C] -> the first index of the row maximum, a NaN counting as -inf (all NaN: 0)."""
    return np.where(np.isnan(v), -np.inf, v).argmax(axis=1)


def _seq_sum(terms, dt):
    """Sum over the LAST axis in index order in `dt` (float64: numpy's own sum)."""
    if dt == np.float64:
        return terms.sum(axis=-1)
    s = np.zeros(terms.shape[:-1], dtype=dt)
    for k in range(terms.shape[-1]):
        s = (s + terms[..., k]).astype(dt)
    return s


def rectify_ref(F, P, eta, n, temp, thr, family, dt, mistake=None):
    """F [M, D] and P [M, ldp] hold exactly the values of the device buffers.  -> dict(out [M, ldp] dt, conf [M], arg, argp [M], lab [M] uint8,
    changed int)."""
    with np.errstate(all="ignore"):
        F, eta = np.asarray(F).astype(dt), np.asarray(eta).astype(dt)
        Pd = np.asarray(P).astype(dt)
        n = np.asarray(n)
        C = len(n)
        M = F.shape[0]
        seen = n > 0
        out = Pd.copy()
        if seen.any():
            d = np.zeros((M, C), dtype=dt)
            for c in np.nonzero(seen)[0]:
                diff = (F - eta[c][None, :]).astype(dt)
                s = _seq_sum((diff * diff).astype(dt), dt)
                d[:, c] = s if mistake == "no_root" else np.sqrt(s).astype(dt)
            dmin = np.fmin.reduce(np.where(seen[None, :], d, np.inf), axis=1).astype(dt)
            d = np.where(seen[None, :], d, dt(0) if mistake == "unseen_at_zero" else dmin[:, None]).astype(dt)
            z = (-(d - dmin[:, None]).astype(dt) / dt(temp)).astype(dt)
            if family == 0:
                r = (np.exp(z).astype(dt) * Pd[:, :C]).astype(dt)
                if mistake == "unseen_weight_zero":
                    r = np.where(seen[None, :], r, dt(0))
                out[:, :C] = r if mistake == "no_renorm" else (r / _seq_sum(r, dt)[:, None]).astype(dt)
            else:
                o = (Pd[:, :C] + z).astype(dt)
                if mistake == "unseen_weight_zero":
                    o = np.where(seen[None, :], o, -np.inf)
                out[:, :C] = o
        o = out[:, :C]
        arg, argp = first_argmax(o), first_argmax(Pd[:, :C])
        mx = np.where(np.isnan(o), -np.inf, o).max(axis=1).astype(dt)
        if family == 0:
            conf = mx
        else:
            conf = (dt(1) / _seq_sum(np.exp((o - mx[:, None]).astype(dt)).astype(dt), dt)).astype(dt)
        keep = ~np.isnan(o).any(axis=1) & (conf > dt(np.float32(thr)))
        lab = np.where(keep, arg, 255).astype(np.uint8)
        return dict(out=out, conf=conf, arg=arg, argp=argp, lab=lab, changed=int((arg != argp).sum()))


def accumulate_ref(F, lab, C, dt):
    """-> (S [C, D] dt: the sums in cell order, per part of PART_CELLS cells and then the parts in order; cnt [C] int64)."""
    F = np.asarray(F).astype(dt)
    M, D = F.shape
    S = np.zeros((C, D), dtype=dt)
    for p0 in range(0, M, PART_CELLS):
        part = np.zeros((C, D), dtype=dt)
        for m in range(p0, min(M, p0 + PART_CELLS)):
            if lab[m] < C:
                part[lab[m]] = (part[lab[m]] + F[m]).astype(dt)
        S = (S + part).astype(dt)
    return S, np.array([int((np.asarray(lab) == c).sum()) for c in range(C)], dtype=np.int64)


def alpha(momentum, n, dt=np.float64):
    """a = max(1 - M, 1 / (n + 1)); float32: (float)(1.0 - M) and 1.f / (float)(n + 1)."""
    if dt == np.float32:
        return max(np.float32(1.0 - momentum), np.float32(np.float32(1) / np.float32(n + 1)))
    return max(1.0 - momentum, 1.0 / (n + 1))


def update_ref(S, cnt, eta, n, momentum, dt, mistake=None, cells=None):
    """-> (eta' [C, D] dt, n' [C] int32)."""
    eta2, n2 = np.asarray(eta).astype(dt).copy(), np.asarray(n).astype(np.int32).copy()
    for c in range(len(n2)):
        if cnt[c] == 0:
            continue
        mean = (S[c] / dt(cells if mistake == "mean_over_cells" else cnt[c])).astype(dt)
        if n2[c] == 0:
            eta2[c] = mean
        else:
            a = dt(alpha(1.0 - momentum if mistake == "momentum_swapped" else momentum, int(n2[c]), dt))
            eta2[c] = (eta2[c] + (a * (mean - eta2[c]).astype(dt)).astype(dt)).astype(dt)
        n2[c] += 1
    return eta2, n2


def step_ref(case, dt, lab=None, mistake=None):
    """rectify -> accumulate -> update on a case of make_case.  `lab`: the labels accumulate reads (None: rectify's own)."""
    k = case
    r = rectify_ref(k["F"], k["P"], k["eta"], k["n"], k["temp"], k["thr"], k["family"], dt, mistake)
    used = r["lab"] if lab is None else np.asarray(lab)
    S, cnt = accumulate_ref(k["F"], used, k["C"], dt)
    eta2, n2 = update_ref(S, cnt, k["eta"], k["n"], k["momentum"], dt, mistake, cells=k["F"].shape[0])
    if mistake == "update_first":          # the batch labelled with prototypes that already hold it
        r = rectify_ref(k["F"], k["P"], eta2, n2, k["temp"], k["thr"], k["family"], dt)
    return dict(r, S=S, cnt=cnt, eta=eta2, n=n2)


def make_case(M, D, C, bf16=False, family=0, ldp=None, ldF=None, seed=0, unseen=2, temp=1.0, thr=0.6, momentum=0.9):
    """Prototypes at pairwise distance >= 4, features at noise 0.5 per channel around the prototype of a drawn class, a teacher that is right
    about four cells in five.  F holds the stored values (bf16-rounded when bf16) as float32 [M, ldF]; columns D .. ldF-1 and the columns
    C .. ldp-1 of P are junk no launch may use.  `unseen` classes have n = 0 and a row of eta that is never to be read (NaN)."""
    rng = np.random.default_rng(1000 + seed)
    ldp, ldF = ldp or C, ldF or D
    proto = rng.standard_normal((C, D))
    gap = min(np.linalg.norm(proto[a] - proto[b]) for a in range(C) for b in range(a))
    proto *= max(1.0, 4.0 / gap)
    truth = rng.integers(0, C, size=M)
    F = rng.standard_normal((M, ldF)).astype(np.float32) * 100.0
    F[:, :D] = (proto[truth] + 0.5 * rng.standard_normal((M, D))).astype(np.float32)
    if bf16:
        F = to_bf16(F)
    says = np.where(rng.random(M) < 0.8, truth, rng.integers(0, C, size=M))
    v = 1.5 * rng.standard_normal((M, C))
    v[np.arange(M), says] += 3.0
    P = rng.standard_normal((M, ldp)).astype(np.float32) * 7.0
    if family == 0:
        e = np.exp(v - v.max(axis=1, keepdims=True))
        P[:, :C] = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    else:
        P[:, :C] = v.astype(np.float32)
    n = rng.integers(1, 30, size=C).astype(np.int32)
    eta = (proto + 0.05 * rng.standard_normal((C, D))).astype(np.float32)
    if unseen:
        gone = rng.choice(C, size=min(unseen, C - 1), replace=False)
        n[gone] = 0
        eta[gone] = np.nan
    return dict(F=F, P=P, eta=eta, n=n, C=C, D=D, ldp=ldp, ldF=ldF, M=M, bf16=bf16, family=family, temp=float(np.float32(temp)),
                thr=float(np.float32(thr)), momentum=momentum, truth=truth)


def features(case):
    """The D used columns of F."""
    return case["F"][:, :case["D"]]


def _core(case):
    return dict(case, F=features(case))


def bar(ref32, ref64):
    fin = np.isfinite(ref64)
    err32 = float(np.abs(ref32.astype(np.float64) - ref64)[fin].max()) if fin.any() else 0.0
    return FACTOR * err32 + REL * float(np.abs(ref64[fin]).max() if fin.any() else 0.0), err32


def excluded(ref64, case, b):
    """The cells whose label or arg-max the bar cannot decide: float64 top two of out within EXCL * b, or conf within EXCL * b of thr.  A cell
    with a NaN in its float64 row is decided (255) and never excluded."""
    o = ref64["out"][:, :case["C"]]
    nan = np.isnan(o).any(axis=1)
    top = np.sort(np.where(np.isnan(o), -np.inf, o), axis=1)
    with np.errstate(invalid="ignore"):
        near = (top[:, -1] - top[:, -2] <= EXCL * b) | (np.abs(ref64["conf"] - case["thr"]) <= EXCL * b)
    return near & ~nan


def check_step(got, case, report=None):
    """got: dict(out [M, ldp], lab [M], changed (the sum of changed_part), S [C, D], cnt [C], eta [C, D], n [C]) of the three launches on the
    case's stored inputs.  AssertionError names the first quantity outside its bar.  -> dict of gpu_err / err32 ratios (and prints them when
    `report` is a string)."""
    k = _core(case)
    C = k["C"]
    r64, r32 = step_ref(k, np.float64), step_ref(k, np.float32)
    ratios = {}
    # out
    b_out, e32 = bar(r32["out"][:, :C], r64["out"][:, :C])
    go = np.asarray(got["out"], dtype=np.float64)
    assert go.shape == r64["out"].shape, (go.shape, r64["out"].shape)
    assert np.array_equal(np.asarray(got["out"])[:, C:].view(np.uint32), np.asarray(case["P"])[:, C:].view(np.uint32)), "out: the columns behind C are not P's"
    nanref = np.isnan(r64["out"][:, :C])
    assert np.array_equal(np.isnan(go[:, :C]), nanref), "out: NaN where the contract has a number, or a number where it has NaN"
    err = float(np.abs(go[:, :C] - r64["out"][:, :C])[~nanref].max()) if (~nanref).any() else 0.0
    ratios["out"] = err / e32 if e32 else 0.0
    assert err <= b_out, f"out: error {err:.3e} beyond the bar {b_out:.3e} (err32 {e32:.3e})"
    # the discrete outputs
    ex = excluded(r64, k, b_out)
    share = float(ex.mean())
    assert share <= CAP, f"{share:.3%} of the cells are excluded from the discrete comparison (cap {CAP:.0%})"
    lab = np.asarray(got["lab"])
    bad = (lab != r64["lab"]) & ~ex
    assert not bad.any(), f"lab: {int(bad.sum())} cells differ outside the exclusions, first {int(np.nonzero(bad)[0][0])}"
    lo = int(((r64["arg"] != r64["argp"]) & ~ex).sum())
    assert lo <= int(got["changed"]) <= lo + int(ex.sum()), f"changed: {int(got['changed'])}, expected {lo} (+ at most {int(ex.sum())} excluded)"
    # the sums and the prototypes, from the labels the device made
    s64, s32 = step_ref(k, np.float64, lab=lab), step_ref(k, np.float32, lab=lab)
    assert np.array_equal(np.asarray(got["cnt"]).astype(np.int64), s64["cnt"]), (got["cnt"], s64["cnt"])
    assert np.array_equal(np.asarray(got["n"]).astype(np.int64), s64["n"].astype(np.int64)), (got["n"], s64["n"])
    for name in ("S", "eta"):
        live = np.ones(C, dtype=bool) if name == "S" else (s64["cnt"] > 0) | (np.asarray(k["n"]) > 0)      # an unseen, absent class: its row is untouched junk
        b, e32 = bar(s32[name][live], s64[name][live])
        g = np.asarray(got[name], dtype=np.float64)[live]
        assert np.isfinite(g).all(), f"{name}: not finite"
        err = float(np.abs(g - s64[name][live]).max())
        ratios[name] = err / e32 if e32 else 0.0
        assert err <= b, f"{name}: error {err:.3e} beyond the bar {b:.3e} (err32 {e32:.3e})"
    gone = (s64["cnt"] == 0)
    assert np.array_equal(np.asarray(got["eta"])[gone].view(np.uint32), np.asarray(case["eta"])[gone].view(np.uint32)), "eta: a class absent from the batch moved"
    if report is not None:
        print(f"proto {report}: gpu_err / err32  out {ratios['out']:.3f}  S {ratios['S']:.3f}  eta {ratios['eta']:.3f}  excluded {int(ex.sum())} of {len(ex)}")
    return ratios


def as_got(r, case):
    """A step_ref result in the shape check_step takes (the float32 restatement standing in for the device)."""
    return dict(out=r["out"].astype(np.float32), lab=r["lab"], changed=r["changed"], S=r["S"], cnt=r["cnt"], eta=r["eta"].astype(np.float32), n=r["n"])


# the shapes the CPU and GPU tests share: (M, D, C) and what each one is there for
CASES = {
    "bf16_2x5x7_2048_19": dict(M=2 * 5 * 7, D=2048, C=19, bf16=True),                  # the row-in-registers path at a non-power-of-two M
    "f32_3x9x9_1024_19": dict(M=3 * 9 * 9, D=1024, C=19, seed=1),
    "f32_2x8x16_256_25_logits": dict(M=2 * 8 * 16, D=256, C=25, family=1, ldp=28, seed=2),      # family 1, padded rows
    "f32_1x3x3_8_2": dict(M=1 * 3 * 3, D=8, C=2, unseen=0, seed=3),                    # the minimum
    "f32_2x9x9_64_64_ld72": dict(M=2 * 9 * 9, D=64, C=64, ldF=72, seed=4),             # every lane a class, padded feature rows
    "bf16_3x11x11_128_19_parts": dict(M=3 * 11 * 11, D=128, C=19, bf16=True, seed=5),  # M above one accumulate part: the partial order
    "bf16_1x6x7_4096_5_wide": dict(M=1 * 6 * 7, D=4096, C=5, bf16=True, unseen=1, seed=6),      # D above the registers: the second read of the row
}
_MADE = {}


def case(name):
    """make_case(**CASES[name]), made once and shared (read-only)."""
    if name not in _MADE:
        _MADE[name] = make_case(**CASES[name])
    return _MADE[name]
