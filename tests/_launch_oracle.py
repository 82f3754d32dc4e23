"""Float64 oracle for ONE recorded launch of a plan's LaunchList (simt_amd/engine.py), driven by its descriptor / arguments.

A check reads the launch's operands through the device pointers it was given, restates the semantics documented in
include/simt_hip.h in float64 (shifted / gathered matmuls on the device: test infrastructure, the product never calls a
vendor GEMM), and compares them with what the kernel stored.  Used by tests/test_gpu_plan_launches.py, _v2.py (the benchmarked bf16
plans) and _small.py (small odd-shaped plans, fp32 and bf16); tests/test_launch_oracle_cpu.py runs the fp32 forms on CPU tensors:

    chk = prepare(item, mem)      # snapshot the inputs, poison the outputs (NaN; pitch columns with a sentinel)
    <run the launch>
    got = chk.outputs()           # fresh copies of what the kernel stored
    recs = chk.check(got)         # AssertionError on a violation; else [(tag, shape, worst error / bound)]

The bars:
  * bf16 outputs: `tight_bf16` (1 bf16 ulp + fp32 accumulation slack for every element, >= 99.5 % exactly the rounded
    float64 result where the output has at least 2048 elements; the storage-format bar of round 5);
  * the same outputs in fp32 storage: `tight_f32_ratio`, the same derivation with the final rounding 2^-22 |ref| in place of the bf16 ulp, the
    accumulation term unchanged, no exact share (`tight_ratio` picks the form from the stored dtype);
  * fp32 outputs and per-slot fp32 partial sums: `fp32_sum_bound`, the form of test_wgrad_production_shapes_bf16's bound;
  * data movement (pools, scatters, im2col, packing, slab reduces): bit-exact against a restatement of the same arithmetic.

Conv outputs are checked on a sampled set of pixel rows (`conv_rows`); statistics and BatchNorm sums on whole columns (the direct stem's
statistics slot by slot: each is one 8 x 32 output tile).
Launches that carry a fused BatchNorm (simt_conv_desc.fbn) are refused: run the plans with SIMT_BN_GRID=0.
"""
import ctypes as C

import torch
import torch.nn.functional as F

from simt_amd import _lib as L

BF = torch.bfloat16
F64 = torch.float64
U = 2.0 ** -24                 # unit roundoff of fp32
GEMM_FLOPS = [0.0]             # float64 multiply-adds x 2 done by conv_ref / wgrad_ref (the oracle's cost, reported by the tests)
SENTINEL = -12288.0            # exactly representable in bf16 and fp32: written into pitch columns a kernel must leave alone


# ---- the bf16 per-op bar, tied to the STORAGE FORMAT (round 5) ---------------------------------------------------------------------------
# `_rel < 1e-2 of max|ref|` is 10-50x looser than one bf16 ulp of a typical element: round 4's stale-dword store bug passed it.  Here every
# element is compared with the float64 result of the same op on the same bf16 operands:
#     |got - ref| <= 1 ulp_bf16(ref) + 16 * sqrt(K) * 2^-24 * rms(ref)        (one rounding of an fp32 sum of K products)
# for EVERY element, and got == bf16(ref) exactly for at least `exact_min` of them (what is left are round-to-nearest ties decided by the
# last bits of the fp32 sum).  ulp_bf16(v) = 2^(floor(log2 |v|) - 7), floored at the ulp of rms * 2^-6 so that near-zero results are held to
# the accumulation slack, not to a vanishing ulp.
def ulp_bf16(ref64, floor_at):
    mag = ref64.abs().clamp_min(floor_at)
    return torch.exp2(torch.floor(torch.log2(mag)) - 7.0)


def _tight_tol(ref64, K, inner64=None):
    rms = ref64.pow(2).mean().sqrt().item()
    tol = ulp_bf16(ref64, rms * 2.0 ** -6) + 16.0 * (K ** 0.5) * 2.0 ** -24 * rms
    if inner64 is not None:
        tol = tol + ulp_bf16(inner64, inner64.pow(2).mean().sqrt().item() * 2.0 ** -6)
    return tol


def tight_bf16(got_bf16, ref64, K, what, exact_min=0.995, inner64=None, alt64=None):
    """got: bf16 tensor as stored by the kernel; ref64: float64 result before the final rounding (same shape, same device).
    inner64: for the epilogues that ROUND TWICE -- the conv kernels park the accumulators as a bf16 tile in LDS and apply bias / residual /
    ReLU to the parked values on the way out (what unfused bf16 PyTorch ops do: the conv's output tensor is bf16 before `+= residual`) -- the
    float64 conv result before that FIRST rounding; ref64 is then computed by the caller from bf16(inner64).  Where the fp32 sum and the
    float64 sum round to different bf16 neighbours (rare: decided by the last bits of the sum) the output moves by one ulp OF THE CONV RESULT,
    which after a cancelling residual can be many ulps of the output: one such ulp is added to the bound.
    alt64: a second admissible reference for the elements where it is not NaN (a ReLU mask whose sign an fp32 evaluation may decide either
    way, see relu_sign): the element passes if it is within the bound of either.  Returns the exactly-rounded fraction."""
    exact, _ = tight_bf16_ratio(got_bf16, ref64, K, what, exact_min, inner64, alt64)
    return exact


EXACT_SHARE_MIN_ELEMS = 2048   # below this an output is held to the per-element bound only (see tight_bf16_ratio)


def _keep(keep, tol):
    """keep = (dict, key): hand the bound tensor of a bar back to the handler's `bounds` (the red tests move an element by a multiple of it)."""
    if keep is not None:
        keep[0][keep[1]] = tol


def tight_bf16_ratio(got_bf16, ref64, K, what, exact_min=0.995, inner64=None, alt64=None, keep=None):
    """tight_bf16, also returning the worst |got - ref| / bound.  An output of fewer than EXACT_SHARE_MIN_ELEMS elements is held to the
    per-element bound only: the exact share is a statement about a population (the rounding model predicts about sqrt(K) 2^-16 of the
    elements on a tie), and on a few hundred elements one tie more or less moves the share by more than the cap's margin.  The cap itself
    (`exact_min`) is never lowered."""
    assert got_bf16.dtype == BF and ref64.dtype == F64 and got_bf16.shape == ref64.shape
    g = got_bf16.double()
    tol = _tight_tol(ref64, K, inner64)
    _keep(keep, tol)
    err = (g - ref64).abs()
    ok_exact = got_bf16 == ref64.float().to(BF)
    if alt64 is not None:
        has = ~torch.isnan(alt64)
        err = torch.where(has, torch.minimum(err, (g - alt64).abs()), err)
        ok_exact = ok_exact | (has & (got_bf16 == alt64.float().to(BF)))
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    bad = err > tol
    nbad = int(bad.sum().item())
    ratio = (err / tol).max().item() if err.numel() else 0.0
    exact = ok_exact.double().mean().item() if err.numel() else 1.0
    assert nbad == 0, (f"{what}: {nbad} of {bad.numel()} elements off by more than 1 bf16 ulp + fp32 accumulation slack (worst "
                       f"{ratio:.1f} x the bound; first at {bad.nonzero()[0].tolist()})")
    if err.numel() >= EXACT_SHARE_MIN_ELEMS:
        assert exact >= exact_min, f"{what}: only {exact:.5f} of the elements equal the float64 result rounded to bf16 (bar {exact_min})"
    return exact, ratio


def tight_f32_ratio(got_f32, ref64, K, what, alt64=None, keep=None):
    """The fp32-STORAGE form of tight_bf16, by the same derivation: the final rounding is 2^-22 |ref| (the margin prepare_conv and
    fp32_sum_bound use for a stored fp32 value) in place of one bf16 ulp, the accumulation term 16 sqrt(K) 2^-24 rms(ref) is unchanged, and
    there is no exact-share requirement (fp32 storage keeps the last bits of the fp32 evaluation, which the float64 reference does not
    predict).  No second rounding either: an fp32 tile parked in LDS is the accumulator itself.  alt64 as in tight_bf16: where it is not
    NaN the element passes within the bound of either reference (the final rounding taken of the larger of the two)."""
    assert got_f32.dtype == torch.float32 and ref64.dtype == F64 and got_f32.shape == ref64.shape
    g = got_f32.double()
    rms = ref64.pow(2).mean().sqrt().item() if ref64.numel() else 0.0
    mag = ref64.abs()
    err = (g - ref64).abs()
    if alt64 is not None:
        has = ~torch.isnan(alt64)
        err = torch.where(has, torch.minimum(err, (g - alt64).abs()), err)
        mag = torch.where(has, torch.maximum(mag, alt64.abs()), mag)
    tol = 2.0 ** -22 * mag + 16.0 * (K ** 0.5) * U * rms
    _keep(keep, tol)
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    bad = err > tol
    nbad = int(bad.sum().item())
    ratio = (err / tol.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    assert nbad == 0, (f"{what}: {nbad} of {bad.numel()} elements off by more than 2^-22 |ref| + fp32 accumulation slack (worst "
                       f"{ratio:.1f} x the bound; first at {bad.nonzero()[0].tolist()})")
    return 1.0, ratio


def tight_ratio(got, ref64, K, what, exact_min=0.995, inner64=None, alt64=None, keep=None):
    """The storage-format bar of `got`'s dtype: tight_bf16_ratio for bf16, tight_f32_ratio for fp32."""
    if got.dtype == BF:
        return tight_bf16_ratio(got, ref64, K, what, exact_min, inner64, alt64, keep)
    return tight_f32_ratio(got, ref64, K, what, alt64, keep)


def fp32_sum_bound(terms_abs, R, ref64):
    """Bound on |fp32 result - float64 sum| for per-column sums that the kernel forms as fp32 partials over blocks of at most R consecutive rows
    (a statistics slot, a BatchNorm-backward block, a weight-gradient split, a column-sum row range), the partials then added in float64 (by the
    kernel's finalize or by this checker) and the total rounded once to fp32 where it is stored as fp32.

    terms_abs: [M, C] float64 |a_i| of the summed terms.  In block k (A_k = sum of |a_i| over its rows) an fp32 sum of n <= R terms in ANY order
    makes at most n - 1 roundings, each |delta| <= 2^-24 * |partial| <= 2^-24 * A_k.  The roundings of round-to-nearest are modelled, as in
    test_wgrad_production_shapes_bf16's bound `16 sqrt(M) 2^-24 rms(ref) + 2^-22 |ref|`, as independent and zero-mean, with the same safety factor
    16 on their standard deviation:
        |got - ref| <= 16 * 2^-24 * sqrt(R) * sqrt(sum_k A_k^2)  +  2^-22 * |ref|
    (the second term: the final fp32 rounding of the stored value with margin).  With one block (R >= M) and A = sqrt(M) rms this IS the wgrad
    bound.  The worst case (R - 1) 2^-24 sum_k A_k is never smaller, so this is the tighter of the two."""
    M = terms_abs.shape[0]
    R = max(1, int(R))
    nb = -(-M // R)
    pad = nb * R - M
    t = terms_abs if pad == 0 else torch.cat([terms_abs, terms_abs.new_zeros((pad,) + tuple(terms_abs.shape[1:]))])
    A = t.reshape((nb, R) + tuple(t.shape[1:])).sum(1)
    return 16.0 * U * (R ** 0.5) * A.pow(2).sum(0).sqrt() + 2.0 ** -22 * ref64.abs()


def fp32_bar(got, ref64, tol, what, keep=None):
    """Element-wise |got - ref| <= tol (tol: tensor or scalar); returns the worst ratio."""
    err = (got.double() - ref64).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    tol = torch.as_tensor(tol, dtype=F64, device=err.device).expand_as(err).clamp_min(1e-300)
    _keep(keep, tol)
    ratio = (err / tol).max().item() if err.numel() else 0.0
    bad = err > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the fp32 bound (worst {ratio:.2f} x; first at {bad.nonzero()[0].tolist()})"
    return ratio


def exact_bar(got, ref, what):
    """Bit-exact (NaN-aware through the bit pattern)."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if got.dtype.is_floating_point:
        eq = got.view(torch.int16 if got.element_size() == 2 else torch.int32) == ref.view(torch.int16 if ref.element_size() == 2 else torch.int32)
        # +0 / -0 are the same value for every consumer
        eq = eq | ((got == 0) & (ref == 0))
    else:
        eq = got == ref
    nbad = int((~eq).sum().item())
    assert nbad == 0, f"{what}: {nbad} of {eq.numel()} elements differ from the exact result (first at {(~eq).nonzero()[0].tolist()})"
    return 0.0


def relu_sign(y, scale, shift):
    """ReLU mask `y * scale + shift > 0` of a bf16 y with fp32 constants, as the kernels evaluate it in fp32 -- fused (one rounding: the sign
    of the exact value, which float64 gives exactly since y * scale is exact there) or as a multiply then an add (two roundings: the sign may
    differ where |y * scale + shift| is within 2^-23 (|y * scale| + |shift|)).  Returns (mask, ambiguous)."""
    a = y.double() * scale.double()
    v = a + shift.double()
    amb = v.abs() <= 2.0 ** -23 * (a.abs() + shift.double().abs())
    return v > 0, amb


def unpack_bits(bits, M, Cn):
    b = bits.reshape(M, Cn // 8).to(torch.int32)
    return ((b.unsqueeze(-1) >> torch.arange(8, device=bits.device, dtype=torch.int32)) & 1).reshape(M, Cn).bool()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# device memory: raw pointers -> views of the tensors that own them
# ---------------------------------------------------------------------------------------------------------------------------------------------
class Mem:
    """Every tensor a plan owns, by address range: a descriptor pointer becomes a flat VIEW (reads see the buffer, poisoning writes it)."""

    def __init__(self, tensors):
        spans = {}
        for t in tensors:
            if not isinstance(t, torch.Tensor) or t.numel() == 0:
                continue
            base = t.untyped_storage()
            key = base.data_ptr()
            if key not in spans or spans[key][1] < base.nbytes():
                spans[key] = (key, base.nbytes(), t)
        self.spans = sorted(spans.values(), key=lambda s: s[0])
        self.log = None          # while a handler prepares a launch (see prepare): every (address, bytes) it views

    def view(self, ptr, n, dtype):
        """Flat [n] view of dtype at device address ptr."""
        assert ptr, "NULL operand"
        esz = torch.empty((), dtype=dtype).element_size()
        if self.log is not None:
            self.log.append((ptr, n * esz))
        for start, nbytes, t in self.spans:
            if start <= ptr and ptr + n * esz <= start + nbytes:
                raw = torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage(), 0, (nbytes,))
                off = ptr - start
                assert off % esz == 0
                return raw[off:off + n * esz].view(dtype)
        raise KeyError(f"pointer {ptr:#x} (+{n * esz} bytes) is not inside any tensor the plan owns")

    def span_of(self, ptr):
        for start, nbytes, t in self.spans:
            if start <= ptr < start + nbytes:
                return start, nbytes
        raise KeyError(f"{ptr:#x}")


def _overlap(a, b):
    return a[0] < b[0] + b[1] and b[0] < a[0] + a[1]


def extent(v):
    """(address, bytes) a written view covers: whole rows of a pitched [rows, cols] view (its pitch columns included), else the view."""
    esz = v.element_size()
    if v.dim() == 2 and v.stride(1) == 1 and v.stride(0) >= v.shape[1]:
        return v.data_ptr(), v.shape[0] * v.stride(0) * esz
    assert v.is_contiguous(), "written view is neither contiguous nor row-pitched"
    return v.data_ptr(), v.numel() * esz


class Check:
    """One prepared launch: `outs` = {name: (view, poison)} written by the kernel; `fn(got) -> [(tag, shape, ratio)]`.

    For the last-writer trace (tests/_plan_trace.py): `reads` = [(operand name, address, bytes)] -- the activation operands by name (conv
    x / res, weight-gradient dy{i} / x{i}, BatchNorm-backward dz / y), every other range the handler viewed as in{k} (filled by prepare);
    writes() = the extents of `outs`.  `problems` = [(dy name, x name, output name)] of a weight-gradient launch; `jobs` = [(slab read name,
    destination output name)] of a slab reduce."""

    def __init__(self, outs, fn, restore=(), reads=(), problems=(), jobs=(), bounds=None):
        self.outs, self.fn, self.restore = outs, fn, list(restore)
        self.bounds = bounds if bounds is not None else {}     # filled by check(): {name: bound tensor of that output's bar} (+ "rows" of a conv)
        self.reads, self.problems, self.jobs = list(reads), list(problems), list(jobs)

    def writes(self):
        return [(k,) + extent(v) for k, (v, _p) in self.outs.items()]

    def outputs(self):
        return {k: v.clone() for k, (v, _p) in self.outs.items()}

    def check(self, got):
        return self.fn(got)

    def finish(self):
        """Put back what the kernel must NOT have written (pitch columns poisoned with a sentinel), as the plan had it."""
        for view, saved in self.restore:
            view.copy_(saved)


def _poison(outs, ins):
    """NaN (floats) / 0xA5 (bytes) into every output view that does not overlap an input (an output aliasing an input keeps its content)."""
    for k, (v, p) in outs.items():
        if not p:
            continue
        rng = (v.data_ptr(), v.numel() * v.element_size())
        if any(_overlap(rng, r) for r in ins):
            continue
        if v.dtype.is_floating_point:
            v.fill_(float("nan"))
        else:
            v.fill_(0xA5)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# convolution: simt_conv_fprop (fprop, dgrad, every tile variant)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _dt(code):
    return BF if code == L.SIMT_BF16 else torch.float32


def conv_taps_of(d, n=None):
    n = d.ntaps if n is None else n
    return [(int(d.dy[t]), int(d.dx[t])) for t in range(n)]


def conv_rows(d, device, seed=0, nrand=8192, full_below=131072):
    """Sampled output rows of a conv: all of them up to `full_below`, else every row of the first and the last 256 (covering the first and the
    last M-tile of any tile plan), every row for which some tap reads outside the image, and `nrand` further rows drawn without replacement
    (seeded) from the rows not already in that set."""
    B, Ho, Wo = d.B, d.Ho, d.Wo
    M = B * Ho * Wo
    dev = device
    if M <= full_below:
        return torch.arange(M, device=dev)
    m = torch.arange(M, device=dev)
    ho, wo = (m // Wo) % Ho, m % Wo
    edge = torch.zeros(M, dtype=torch.bool, device=dev)
    for (a, b) in conv_taps_of(d):
        iy, ix = ho * d.stride + a, wo * d.stride + b
        edge |= (iy < 0) | (iy >= d.H) | (ix < 0) | (ix >= d.W)
    fixed = edge.clone()
    fixed[:256] = True
    fixed[-256:] = True
    rest = (~fixed).nonzero().squeeze(1)
    g = torch.Generator(device="cpu").manual_seed(seed)
    pick = rest[torch.randperm(rest.numel(), generator=g)[:nrand].to(dev)]
    assert pick.numel() == min(nrand, rest.numel())
    return torch.cat([fixed.nonzero().squeeze(1), pick]).sort().values


def conv_gather(x4, d, rows):
    """[len(rows), ntaps * Cin] float64 operand rows x[b, ho*stride + dy, wo*stride + dx, :] (zero outside the image), tap-major."""
    B, H, W, Cin = x4.shape
    Ho, Wo = d.Ho, d.Wo
    b, ho, wo = rows // (Ho * Wo), (rows // Wo) % Ho, rows % Wo
    xf = x4.reshape(B * H * W, Cin)
    cols = []
    for (a, c) in conv_taps_of(d):
        iy, ix = ho * d.stride + a, wo * d.stride + c
        ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
        src = (b * H + iy.clamp(0, H - 1)) * W + ix.clamp(0, W - 1)
        cols.append(xf[src].double() * ok.unsqueeze(1))
    return torch.cat(cols, 1)


def conv_ref(x4, w2, d, rows, chunk=16384):
    """float64 sum_{t,ci} x[pixel(m) * stride + tap][ci] * w[n][t * Cin + ci] for the given rows -> [len(rows), w2.shape[0]]."""
    wd = w2.double()
    out = []
    GEMM_FLOPS[0] += 2.0 * rows.numel() * w2.shape[1] * w2.shape[0]
    for i in range(0, rows.numel(), chunk):
        out.append(conv_gather(x4, d, rows[i:i + chunk]) @ wd.t())
    return torch.cat(out) if out else wd.new_zeros(0, w2.shape[0])


def prepare_conv(it, mem, seed=0):
    d = it.keep
    assert not d.fbn, f"{it.tag}: fused BatchNorm launch (run the plan with SIMT_BN_GRID=0)"
    assert not d.w_frag, f"{it.tag}: fragment-ordered weights are an ablation-build experiment"
    lib = L.load()
    B, H, W, Cin, Ho, Wo, Cout = d.B, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout
    M, K = B * Ho * Wo, d.ntaps * Cin
    tin, tout = _dt(d.dtype_in), _dt(d.dtype_out)
    ldy, Nst = d.ldy, d.Nstore
    x = mem.view(d.x, B * H * W * Cin, tin).view(B, H, W, Cin)
    w = mem.view(d.w, d.Npad * K, tin).view(d.Npad, K)
    ins = [(d.x, B * H * W * Cin * x.element_size()), (d.w, d.Npad * K * w.element_size())]
    snap = {"x": x, "w": w}                                                   # views; cloned below where an output may alias them
    reads = [("x", d.x, ins[0][1]), ("w", d.w, ins[1][1])]
    if d.bias:
        snap["bias"] = mem.view(d.bias, Cout, torch.float32).clone()
    if d.res:
        r = mem.view(d.res, M * d.ldr, tin).view(M, d.ldr)
        snap["res"] = r[:, :Nst].clone()
        ins.append((d.res, M * d.ldr * r.element_size()))
        reads.append(("res", d.res, M * d.ldr * r.element_size()))
    if d.res_bits:
        snap["res_bits"] = unpack_bits(mem.view(d.res_bits, M * d.ldr // 8, torch.uint8), M, d.ldr)[:, :Nst].clone()
        reads.append(("res_bits", d.res_bits, M * d.ldr // 8))
    if d.mask:
        mk = mem.view(d.mask, M * d.ldm, tin).view(M, d.ldm)
        snap["mask"] = mk[:, :Nst].clone()
        ins.append((d.mask, M * d.ldm * mk.element_size()))
        reads.append(("mask", d.mask, M * d.ldm * mk.element_size()))
    if d.in_scale:
        snap["in_scale"] = mem.view(d.in_scale, Cin, torch.float32).clone()
        snap["in_shift"] = mem.view(d.in_shift, Cin, torch.float32).clone()
    if d.bnr_mode:
        snap["bnr_y"] = mem.view(d.bnr_y, M * d.bnr_ld, tin).view(M, d.bnr_ld)[:, :Cout].clone()
        reads.append(("bnr_y", d.bnr_y, M * d.bnr_ld * snap["bnr_y"].element_size()))
        snap["bnr_mean"], snap["bnr_rstd"] = (mem.view(p, Cout, torch.float32).clone() for p in (d.bnr_mean, d.bnr_rstd))
        if d.bnr_mode == 2:
            snap["bnr_scale"], snap["bnr_shift"] = (mem.view(p, Cout, torch.float32).clone() for p in (d.bnr_scale, d.bnr_shift))
        else:
            snap["bnr_bits"] = unpack_bits(mem.view(d.bnr_bits, M * Cout // 8, torch.uint8), M, Cout).clone()
            reads.append(("bnr_bits", d.bnr_bits, M * Cout // 8))
    yfull = mem.view(d.y, M * ldy, tout).view(M, ldy)
    outs = {"y": (yfull[:, :Nst], True)}
    restore = []
    if Nst < ldy:                           # pitch columns: a sentinel that must survive, the plan's content put back afterwards
        pc = yfull[:, Nst:]
        restore.append((pc, pc.clone()))
    if d.stats:
        nsl = -(-M // 128)
        outs["stats"] = (mem.view(d.stats, nsl * 2 * Cout, torch.float32).view(nsl, 2, Cout), True)
    mtiles = lib.simt_conv_mtiles(C.byref(d))
    if d.bnr_mode:
        assert mtiles > 0
        outs["bnr"] = (mem.view(d.bnr_part, mtiles * 3 * Cout, torch.float32).view(mtiles, 3, Cout), True)
    if d.in_scale:
        outs["in_out"] = (mem.view(d.in_out, B * H * W * Cin, tin).view(B * H * W, Cin), True)
    # inputs the outputs may alias: copy them now
    for k in ("x", "w"):
        for (o, _p) in outs.values():
            if _overlap((snap[k].data_ptr(), snap[k].numel() * snap[k].element_size()), (o.data_ptr(), o.numel() * o.element_size())):
                snap[k] = snap[k].clone()
    _poison(outs, ins)
    for (pc, _saved) in restore:
        pc.fill_(SENTINEL)
    rows = conv_rows(d, x.device, seed=seed)
    shape = it.shape or f"M{M} N{Cout} K{K}"
    bounds = {"rows": rows}

    def fn(got):
        recs = []
        y = got["y"]
        for (pc, _saved) in restore:
            assert bool((pc == SENTINEL).all()), f"{it.tag} {shape}: columns [Nstore, ldy) were written"
        xin = snap["x"]
        if d.in_scale:                     # operand path: a = relu(x * in_scale + in_shift), rounded to bf16, also written to in_out
            a64 = torch.relu(snap["x"].reshape(-1, Cin).double() * snap["in_scale"].double() + snap["in_shift"].double())
            e, r = tight_ratio(got["in_out"], a64, 2, f"{it.tag} {shape}: in_out", exact_min=0.999)
            recs.append((it.tag + " [in_out]", shape, r))
            xin = got["in_out"].view(B, H, W, Cin)
        wn = snap["w"][:min(Nst, d.Npad)]
        if wn.shape[0] < Nst:
            wn = torch.cat([wn, wn.new_zeros(Nst - wn.shape[0], K)])
        inner = conv_ref(xin, wn, d, rows)                        # [S, Nst] float64
        two = tout == BF and (d.bias or d.res or d.relu)
        v = inner.float().to(BF).double() if two else inner.clone()
        if d.bias:
            bb = torch.zeros(Nst, dtype=F64, device=v.device)
            bb[:min(Cout, Nst)] = snap["bias"][:min(Cout, Nst)].double()
            v = v + bb
        if d.res:
            rr = snap["res"][rows].double()
            if d.res_bits:
                rr = rr * snap["res_bits"][rows]
            v = v + rr
        if d.relu:
            v = torch.relu(v)
        if d.mask:
            v = v * (snap["mask"][rows] > 0)
        ys = y[rows]
        what = f"{it.tag} {shape}"
        if tout == BF:
            _e, r = tight_bf16_ratio(ys, v, K, what, inner64=inner if two else None, keep=(bounds, "y"))
        else:
            rms = inner.pow(2).mean().sqrt().item()
            tol = 16.0 * (K ** 0.5) * U * rms + 2.0 ** -22 * (inner.abs() + v.abs())
            r = fp32_bar(ys, v, tol, what, keep=(bounds, "y"))
        recs.append((it.tag, shape, r))
        if d.stats:                      # per-slot fp32 sums of the STORED values (statistics come before any bias / ReLU: none in these plans)
            assert not (d.bias or d.res or d.relu or d.mask), f"{what}: statistics with an epilogue are not modelled"
            st = got["stats"].double().sum(0)
            yv = y.double()
            R = -(-M // mtiles) if mtiles else 128
            ref = torch.stack([yv.sum(0), (yv * yv).sum(0)])
            tol = torch.stack([fp32_sum_bound(yv.abs(), R, ref[0]), fp32_sum_bound(yv * yv, R, ref[1])])
            recs.append((it.tag + " [stats]", shape, fp32_bar(st[:, :Cout], ref[:, :Cout], tol[:, :Cout], what + " stats", keep=(bounds, "stats"))))
        if d.bnr_mode:                   # fused first pass of the BatchNorm backward on the stored values
            g = y[:, :Cout].double()
            if d.bnr_mode == 2:
                msk, amb = relu_sign(snap["bnr_y"], snap["bnr_scale"], snap["bnr_shift"])
            else:
                msk, amb = snap["bnr_bits"], torch.zeros_like(snap["bnr_bits"])
            xh = (snap["bnr_y"].double() - snap["bnr_mean"].double()) * snap["bnr_rstd"].double()
            gm = g * msk
            ref = torch.stack([gm.sum(0), (gm * xh).sum(0)])
            R = -(-M // mtiles)
            slack = torch.stack([(g.abs() * amb).sum(0), (g.abs() * xh.abs() * amb).sum(0)])
            tol = torch.stack([fp32_sum_bound(gm.abs(), R, ref[0]), fp32_sum_bound((gm * xh).abs(), R, ref[1])]) + slack
            got_s = got["bnr"].double().sum(0)
            recs.append((it.tag + " [bnr S1/S2]", shape, fp32_bar(got_s[:2], ref, tol, what + " bnr S1/S2")))
            assert bool((got["bnr"][:, 2] == 0).all()), f"{what}: third bnr row not zero"
        return recs
    return Check(outs, fn, restore, reads=reads, bounds=bounds)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# weight gradients
# ---------------------------------------------------------------------------------------------------------------------------------------------
def wgrad_ref(dy2, x4, d, chunk=65536):
    """float64 dW[co][t * Cin + ci] = sum_m dy[m][co] * x[pixel(m) * stride + tap_t][ci] over all M pixels (chunked)."""
    M = dy2.shape[0]
    out = None
    GEMM_FLOPS[0] += 2.0 * M * dy2.shape[1] * d.ntaps * x4.shape[3]
    for i in range(0, M, chunk):
        rows = torch.arange(i, min(M, i + chunk), device=dy2.device)
        part = dy2[i:i + chunk].double().t() @ conv_gather(x4, d, rows)
        out = part if out is None else out + part
    return out


def _wgrad_views(d, mem):
    B, H, W, Cin, Ho, Wo, Cd = d.B, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cd
    M, Kt, ns = B * Ho * Wo, d.ntaps * Cin, d.nsplit
    t = _dt(d.dtype)
    dyv = mem.view(d.dy, M * d.ldd, t).view(M, d.ldd)[:, :Cd]
    x = mem.view(d.x, B * H * W * Cin, t).view(B, H, W, Cin)
    slab = mem.view(d.slab, ns * Cd * Kt, torch.float32).view(ns, Cd, Kt)

    class _D:
        pass
    dd = _D()
    dd.Ho, dd.Wo, dd.stride, dd.ntaps, dd.dy, dd.dx = Ho, Wo, d.stride, d.ntaps, d.dy_, d.dx_
    return dyv, x, slab, dd, M, Kt, ns


def prepare_wgrad_descs(it, descs, mem):
    parts = []
    outs, reads, problems = {}, [], []
    for i, d in enumerate(descs):
        dyv, x, slab, dd, M, Kt, ns = _wgrad_views(d, mem)
        parts.append((dyv, x, dd, M, Kt, ns))                # (views: a weight-gradient launch writes its slab only)
        outs[f"slab{i}"] = (slab, True)
        reads += [(f"dy{i}", d.dy, M * d.ldd * dyv.element_size()), (f"x{i}", d.x, x.numel() * x.element_size())]
        problems.append((f"dy{i}", f"x{i}", f"slab{i}"))
    _poison(outs, [])
    shape = it.shape
    bounds = {}

    def fn(got):
        recs = []
        for i, (dyv, x, dd, M, Kt, ns) in enumerate(parts):
            r64 = wgrad_ref(dyv, x, dd)
            s = got[f"slab{i}"].double().sum(0)
            rms = r64.pow(2).mean().sqrt().item()
            tol = 16.0 * (M ** 0.5) * U * rms + 2.0 ** -22 * r64.abs()
            recs.append((it.tag, f"{shape} [problem {i}: Cd{dyv.shape[1]} K{Kt}]" if len(parts) > 1 else shape,
                         fp32_bar(s, r64, tol, f"{it.tag} {shape} problem {i}: slab sum vs float64 dY^T x", keep=(bounds, f"slab{i}"))))
        return recs
    return Check(outs, fn, reads=reads, problems=problems, bounds=bounds)


def _seq_sum(slab_rows):
    """fp32 sum over the split axis (dim 0) in split order: what the reduce kernels add, bit for bit."""
    s = torch.zeros_like(slab_rows[0])
    for k in range(slab_rows.shape[0]):
        s = s + slab_rows[k]
    return s


def reduce_expect(slab, nsplit, Cd, Ktot, Cin, co_off, tap_off, Cout, RS):
    """dst[co][ci][t] = sum_split slab[split][co_off + co][(tap_off + t) * Cin + ci] (simt_wgrad_reduce)."""
    s3 = slab.view(nsplit, Cd, Ktot)[:, co_off:co_off + Cout, tap_off * Cin:(tap_off + RS) * Cin]
    s = _seq_sum(s3.reshape(nsplit, Cout, RS, Cin))
    return s.permute(0, 2, 1).contiguous()                          # [Cout][Cin][RS]


def prepare_wgrad_reduce(it, mem, jobs):
    """jobs: [(slab ptr, dst ptr, nsplit, Cd, Ktot, Cin, co_off, tap_off, Cout, RS, accumulate)]"""
    outs, exp_in, reads = {}, [], []
    for i, (sp, dp, ns, Cd, Kt, Cin, co, to, Co, RS, acc) in enumerate(jobs):
        reads.append((f"slab{i}", sp, ns * Cd * Kt * 4))
        slab = mem.view(sp, ns * Cd * Kt, torch.float32).clone()
        dst = mem.view(dp, Co * Cin * RS, torch.float32).view(Co, Cin, RS)
        exp_in.append((slab, ns, Cd, Kt, Cin, co, to, Co, RS, dst.clone() if acc else None))
        outs[f"dst{i}"] = (dst, not acc)
    _poison(outs, [])

    def fn(got):
        for i, (slab, ns, Cd, Kt, Cin, co, to, Co, RS, prev) in enumerate(exp_in):
            e = reduce_expect(slab, ns, Cd, Kt, Cin, co, to, Co, RS)
            if prev is not None:
                e = prev + e
            exact_bar(got[f"dst{i}"], e, f"{it.tag} job {i} (co_off {co}, tap_off {to}, Cout {Co}, RS {RS})")
        return [(it.tag, f"{len(jobs)} job(s)", 0.0)]
    return Check(outs, fn, reads=reads, jobs=[(f"slab{i}", f"dst{i}") for i in range(len(jobs))])


def prepare_wgrad_reduce_exp(it, mem):
    slab_p, dst_p, ns, Cd, Cin, QP, row_off, tap_off, Cout, RS = it.args
    slab = mem.view(slab_p, ns * Cd * Cin, torch.float32).view(ns, Cd, Cin).clone()
    dst = mem.view(dst_p, Cout * Cin * RS, torch.float32).view(Cout, Cin, RS)
    outs = {"dst": (dst, True)}
    _poison(outs, [])

    def fn(got):
        rows = (torch.arange(RS, device=slab.device).view(RS, 1) + tap_off) * QP + row_off + torch.arange(Cout, device=slab.device).view(1, Cout)
        s = _seq_sum(slab[:, rows.reshape(-1)].view(ns, RS, Cout, Cin))          # [RS][Cout][Cin]
        exact_bar(got["dst"], s.permute(1, 2, 0).contiguous(), f"{it.tag} (row_off {row_off}, tap_off {tap_off})")
        return [(it.tag, f"Cd{Cd} Cin{Cin} Cout{Cout} RS{RS}", 0.0)]
    return Check(outs, fn, reads=[("slab0", slab_p, ns * Cd * Cin * 4)], jobs=[("slab0", "dst")])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# weight packing
# ---------------------------------------------------------------------------------------------------------------------------------------------
def pack_positions(Cout, Cin, RS, row_off, tap_off, ldk, Ck, mode, device):
    """Flat destination offset of w[co][ci][t] for layout mode 0 / 1 / 2 (csrc/bn_pool.hip pack_weight_kernel), OIHW order."""
    co = torch.arange(Cout, device=device).view(Cout, 1, 1)
    ci = torch.arange(Cin, device=device).view(1, Cin, 1)
    t = torch.arange(RS, device=device).view(1, 1, RS)
    lm = mode & 0xFF
    if lm == 0:
        row, kcol = row_off + co + 0 * ci + 0 * t, (tap_off + t) * Cin + ci + 0 * co
    elif lm == 1:
        row, kcol = ci + 0 * co + 0 * t, (tap_off + t) * Ck + row_off + co + 0 * ci
    else:
        row, kcol = (tap_off + t) * Ck + row_off + co + 0 * ci, ci + 0 * co + 0 * t
    return row, kcol


def prepare_pack(it, mem, jobs, dst_sizes):
    """jobs: [(w ptr, dst ptr, cscale ptr or 0, ldk, Cout, Cin, RS, row_off, tap_off, Ck, mode, dtype)].  Every destination buffer is checked
    WHOLE: the jobs' elements bf16(w) exactly (with a folded scale: bf16 of the float64 product, one rounding, at the K = 1 storage bar), every
    other element still zero (the padding the GEMMs read).  Before the launch the positions the jobs write are poisoned with NaN (the plan's
    constructor has packed them once already); the padding keeps its zeros, which the plan relies on."""
    lib_dt = {L.SIMT_BF16: BF, L.SIMT_F32: torch.float32}
    per_dst = {}
    for j in jobs:
        per_dst.setdefault(j[1], []).append(j)
    outs, plan = {}, []
    for k, (dp, js) in enumerate(per_dst.items()):
        dt = lib_dt[js[0][11]]
        n = dst_sizes(dp, dt)
        view = mem.view(dp, n, dt)
        outs[f"d{k}"] = (view, False)
        exp = torch.zeros(n, dtype=F64, device=view.device)
        written = torch.zeros(n, dtype=torch.bool, device=view.device)
        scaled = torch.zeros(n, dtype=torch.bool, device=view.device)
        for (wp, _dp, cs, ldk, Co, Ci, RS, ro, to, Ck, mode, dtype) in js:
            if mode >> 8:
                raise NotImplementedError("fragment-ordered pack (ablation builds only)")
            w = mem.view(wp, Co * Ci * RS, torch.float32).view(Co, Ci, RS)
            c = mem.view(cs, Co, torch.float32) if cs else None
            row, kcol = pack_positions(Co, Ci, RS, ro, to, ldk, Ck, mode, view.device)
            off = (row * ldk + kcol).reshape(-1)
            assert int(off.max()) < n
            exp[off] = (w.double() * (c.double().view(Co, 1, 1) if c is not None else 1.0)).reshape(-1)
            written[off] = True
            if c is not None:
                scaled[off] = True
        view[written] = float("nan")
        plan.append((f"d{k}", n, dt, len(js), exp, written, scaled))
    bounds = {}

    def fn(got):
        recs = []
        for key, n, dt, njobs, exp, written, scaled in plan:
            g = got[key]
            plain = written & ~scaled
            exact_bar(g[plain], exp[plain].float().to(dt), f"{it.tag} {key}: packed weights")
            exact_bar(g[~written], torch.zeros_like(g[~written]), f"{it.tag} {key}: padding")
            r = 0.0
            if bool(scaled.any()):
                _e, r = tight_ratio(g[scaled], exp[scaled], 1, f"{it.tag} {key}: packed weights x folded BatchNorm scale", exact_min=0.999,
                                    keep=(bounds, key))
            recs.append((it.tag, f"dst {n} elements, {njobs} job(s){' (folded scale)' if bool(scaled.any()) else ''}", r))
        return recs
    return Check(outs, fn, bounds=bounds)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------------------------------------------------------------------------
def prepare_bn_finalize(it, mem):
    part_p, nblk, Cn, count, g_p, b_p, rm_p, rv_p, mom, eps, mean_p, rstd_p, sc_p, sh_p = it.args
    part = mem.view(part_p, nblk * 2 * Cn, torch.float32).view(nblk, 2, Cn).clone()
    gamma = mem.view(g_p, Cn, torch.float32).clone() if g_p else None
    beta = mem.view(b_p, Cn, torch.float32).clone() if b_p else None
    rm = mem.view(rm_p, Cn, torch.float32) if rm_p else None
    rv = mem.view(rv_p, Cn, torch.float32) if rv_p else None
    prev = (rm.clone(), rv.clone()) if rm is not None else None
    outs = {k: (mem.view(p, Cn, torch.float32), True) for k, p in (("mean", mean_p), ("rstd", rstd_p), ("scale", sc_p), ("shift", sh_p))}
    if rm is not None:
        outs["rm"], outs["rv"] = (rm, False), (rv, False)
    _poison(outs, [(part_p, nblk * 2 * Cn * 4)])

    def fn(got):
        s = part.double().sum(0)
        mean = s[0] / count
        var = (s[1] / count - mean * mean).clamp_min(0)
        rstd = 1.0 / (var + eps).sqrt()
        g = gamma.double() if gamma is not None else 1.0
        b = beta.double() if beta is not None else 0.0
        sc = g * rstd
        sh = b - mean * sc
        ulp = 2.0 ** -22                     # two fp32 roundings (the double -> fp32 conversions and fp32 products of the kernel)
        noise = 2.0 ** -45 * part.double().abs().sum(0) / count          # float64 summation-order noise of the two slot sums
        rs = [fp32_bar(got["mean"], mean, ulp * mean.abs() + noise[0], "bn_finalize mean"),
              fp32_bar(got["rstd"], rstd, ulp * rstd.abs(), "bn_finalize rstd"),
              fp32_bar(got["scale"], sc, 2 * ulp * sc.abs(), "bn_finalize scale"),
              fp32_bar(got["shift"], sh, 2 * ulp * (b.abs() if isinstance(b, torch.Tensor) else abs(b)) + 3 * ulp * (mean * sc).abs(),
                       "bn_finalize shift")]
        if prev is not None:
            unb = var * count / (count - 1) if count > 1 else var
            erm = (1 - mom) * prev[0].double() + mom * mean
            erv = (1 - mom) * prev[1].double() + mom * unb
            rs.append(fp32_bar(got["rm"], erm, 3 * ulp * ((1 - mom) * prev[0].double().abs() + mom * mean.abs()), "running_mean"))
            rs.append(fp32_bar(got["rv"], erv, 3 * ulp * ((1 - mom) * prev[1].double().abs() + mom * unb.abs()), "running_var"))
        return [(it.tag, f"C{Cn} slots{nblk} count{count}", max(rs))]
    return Check(outs, fn)


def prepare_bn_apply(it, mem, with_bits):
    a = list(it.args)
    if with_bits:
        y_p, sc_p, sh_p, res_p, y2_p, sc2_p, sh2_p, z_p, bits_p, M, Cn, relu, dtype = a
    else:
        y_p, sc_p, sh_p, res_p, y2_p, sc2_p, sh2_p, z_p, M, Cn, relu, dtype = a
        bits_p = None
    t = _dt(dtype)
    n = M * Cn
    rd = lambda p: mem.view(p, n, t).view(M, Cn).clone()
    y = rd(y_p)
    sc, sh = mem.view(sc_p, Cn, torch.float32).clone(), mem.view(sh_p, Cn, torch.float32).clone()
    res = rd(res_p) if res_p else None
    y2 = rd(y2_p) if y2_p else None
    sc2 = mem.view(sc2_p, Cn, torch.float32).clone() if y2_p else None
    sh2 = mem.view(sh2_p, Cn, torch.float32).clone() if y2_p else None
    outs = {"z": (mem.view(z_p, n, t).view(M, Cn), True)}
    if bits_p:
        outs["bits"] = (mem.view(bits_p, n // 8, torch.uint8).view(M, Cn // 8), True)
    _poison(outs, [])
    bounds = {}

    def fn(got):
        v = y.double() * sc.double() + sh.double()
        K = 2
        if res is not None:
            v, K = v + res.double(), 3
        if y2 is not None:
            v, K = v + y2.double() * sc2.double() + sh2.double(), 5
        if relu:
            v = torch.relu(v)
        _e, r = tight_ratio(got["z"], v, K, f"{it.tag} M{M} C{Cn}", exact_min=0.999, keep=(bounds, "z"))
        if bits_p:
            from_z = (got["z"] > 0).reshape(M, Cn // 8, 8).to(torch.int32)
            exp_bits = (from_z << torch.arange(8, device=from_z.device, dtype=torch.int32)).sum(-1).to(torch.uint8)
            exact_bar(got["bits"], exp_bits, f"{it.tag} M{M} C{Cn}: ReLU bit mask")
        return [(it.tag, f"M{M} C{Cn}{' +res' if res is not None else ''}{' +bn2' if y2 is not None else ''}{' bits' if bits_p else ''}", r)]
    return Check(outs, fn, bounds=bounds)


def prepare_bn_bwd(it, mem):
    d = it.keep
    M, Cn, mm = int(d.M), d.C, d.mask_mode
    t = _dt(d.dtype)
    n = M * Cn
    rd = lambda p: mem.view(p, n, t).view(M, Cn).clone()
    vec = lambda p: mem.view(p, Cn, torch.float32).clone() if p else None
    s = {"dz": rd(d.dz), "y": rd(d.y), "mean": vec(d.mean), "rstd": vec(d.rstd), "scale": vec(d.scale), "shift": vec(d.shift)}
    if mm == 1:
        s["z"] = rd(d.z) > 0
    elif mm == 3:
        s["z"] = unpack_bits(mem.view(d.z, n // 8, torch.uint8), M, Cn).clone()
    if d.y2:
        s.update(y2=rd(d.y2), mean2=vec(d.mean2), rstd2=vec(d.rstd2), scale2=vec(d.scale2))
    lib = L.load()
    own = d.reduce_done_nblk == 0
    nblk = lib.simt_bn_bwd_nblk(M, Cn) if own else d.reduce_done_nblk
    part = mem.view(d.part, nblk * 3 * Cn, torch.float32).view(nblk, 3, Cn)
    outs = {"dy": (mem.view(d.dy, n, t).view(M, Cn), True), "coef": (mem.view(d.coef, 3 * Cn, torch.float32).view(3, Cn), True)}
    if own:
        outs["part"] = (part, True)
    else:
        s["part"] = part.clone()
    for k in ("dy2", "gout", "dgamma", "dbeta", "dgamma2", "dbeta2"):
        p = getattr(d, k)
        if p:
            outs[k] = (mem.view(p, n, t).view(M, Cn), True) if k in ("dy2", "gout") else (mem.view(p, Cn, torch.float32), True)
    ins = [(getattr(d, k), n * s["dz"].element_size()) for k in ("dz", "y") if getattr(d, k)]
    reads = [(k, getattr(d, k), n * s["dz"].element_size()) for k in ("dz", "y", "y2") if getattr(d, k)]
    if mm in (1, 3):
        reads.append(("z", d.z, n * s["dz"].element_size() if mm == 1 else n // 8))
    if not own:
        reads.append(("part", d.part, nblk * 3 * Cn * 4))
    _poison(outs, ins)
    shape = f"M{M} C{Cn} mask{mm}{' +downsample' if d.y2 else ''}{' (reduce in the conv)' if not own else ''}"
    bounds = {}

    def fn(got):
        what = f"{it.tag} {shape}"
        recs = []
        g = s["dz"].double()
        amb = torch.zeros(M, Cn, dtype=torch.bool, device=g.device)
        if mm == 1 or mm == 3:
            msk = s["z"]
        elif mm == 2:
            msk, amb = relu_sign(s["y"], s["scale"], s["shift"])
        else:
            msk = torch.ones_like(amb)
        gm = g * msk
        xh = (s["y"].double() - s["mean"].double()) * s["rstd"].double()
        P = got["part"] if own else s["part"]
        S = P.double().sum(0)                                       # [3][C]
        if own:                                                     # the reduce pass against float64, whole columns
            R = -(-M // nblk)
            refs = [gm.sum(0), (gm * xh).sum(0)]
            tols = [fp32_sum_bound(gm.abs(), R, refs[0]) + (g.abs() * amb).sum(0),
                    fp32_sum_bound((gm * xh).abs(), R, refs[1]) + (g.abs() * xh.abs() * amb).sum(0)]
            if d.y2:
                xh2 = (s["y2"].double() - s["mean2"].double()) * s["rstd2"].double()
                refs.append((gm * xh2).sum(0))
                tols.append(fp32_sum_bound((gm * xh2).abs(), R, refs[2]) + (g.abs() * xh2.abs() * amb).sum(0))
            k = len(refs)
            recs.append((it.tag + " [S1/S2 reduce]", shape, fp32_bar(S[:k], torch.stack(refs), torch.stack(tols), what + " reduce sums", keep=(bounds, "part"))))
        # finalize: coefficients / d gamma / d beta from the slot sums (double), one fp32 rounding
        nco = 3 if d.y2 else 2
        noise = 2.0 ** -45 * P.double().abs().sum(0)                      # float64 summation-order noise of the slot sums
        r = fp32_bar(got["coef"][:nco], S[:nco] / M, 2.0 ** -23 * (S[:nco] / M).abs() + noise[:nco] / M, what + " coef", keep=(bounds, "coef"))
        for k, j in (("dbeta", 0), ("dgamma", 1), ("dbeta2", 0), ("dgamma2", 2)):
            if k in got:
                r = max(r, fp32_bar(got[k], S[j], 2.0 ** -23 * S[j].abs() + noise[j], f"{what} {k}"))
        recs.append((it.tag + " [coef / dgamma / dbeta]", shape, r))
        # apply, with the coefficients the kernel derived (checked above)
        c = got["coef"].double()
        sc = s["scale"].double()

        def ref_dy(gg, xhat, c2):
            return sc * (gg - c[0] - xhat * c2)
        alt = None
        if bool(amb.any()):
            galt = torch.where(amb, g * (~msk), gm)
            alt = torch.where(amb, ref_dy(galt, xh, c[1]), torch.full_like(g, float("nan")))
        _e, r = tight_ratio(got["dy"], ref_dy(gm, xh, c[1]), 4, what + " dy", exact_min=0.999, alt64=alt, keep=(bounds, "dy"))
        recs.append((it.tag + " [dy]", shape, r))
        if d.y2:
            sc = s["scale2"].double()
            xh2 = (s["y2"].double() - s["mean2"].double()) * s["rstd2"].double()
            _e, r = tight_ratio(got["dy2"], ref_dy(gm, xh2, c[2]), 4, what + " dy2", exact_min=0.999, keep=(bounds, "dy2"))
            recs.append((it.tag + " [dy2]", shape, r))
        if "gout" in got:
            exact_bar(got["gout"], gm.to(t), what + " gout")
        return recs
    return Check(outs, fn, reads=reads, bounds=bounds)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# pools, scatters, im2col, column sums, upsampling, tap-expanded head
# ---------------------------------------------------------------------------------------------------------------------------------------------
def maxpool2_expect(y4):
    """MaxPool2d(2, 2) floor mode on NHWC [B, H, W, C]: value and the window index r * 2 + s of the FIRST maximum in scan order (PyTorch's
    rule `val > max || isnan(val)`, the first element always taken; pinned against CPU torch.max_pool2d by test_maxpool2_ties_follow_torch)."""
    B, H, W, Cn = y4.shape
    Hp, Wp = H // 2, W // 2
    v = [y4[:, r:2 * Hp:2, s:2 * Wp:2, :] for r in (0, 1) for s in (0, 1)]
    best, bi = v[0].clone(), torch.zeros(B, Hp, Wp, Cn, dtype=torch.uint8, device=y4.device)
    for k in (1, 2, 3):
        take = (v[k] > best) | torch.isnan(v[k])
        best = torch.where(take, v[k], best)
        bi = torch.where(take, torch.full_like(bi, k), bi)
    return best, bi


def prepare_maxpool2(it, mem):
    y_p, p_p, idx_p, B, H, W, Cn, dtype = it.args
    t = _dt(dtype)
    Hp, Wp = H // 2, W // 2
    y = mem.view(y_p, B * H * W * Cn, t).view(B, H, W, Cn).clone()
    outs = {"p": (mem.view(p_p, B * Hp * Wp * Cn, t).view(B, Hp, Wp, Cn), True),
            "idx": (mem.view(idx_p, B * Hp * Wp * Cn, torch.uint8).view(B, Hp, Wp, Cn), True)}
    _poison(outs, [])

    def fn(got):
        best, bi = maxpool2_expect(y)
        exact_bar(got["p"], best, f"{it.tag} values")
        exact_bar(got["idx"], bi, f"{it.tag} arg-max index (first maximum)")
        return [(it.tag, f"B{B} {H}x{W} C{Cn}", 0.0)]
    return Check(outs, fn)


def maxpool2_bwd_expect(dp, idx, y, H, W):
    B, Hp, Wp, Cn = dp.shape
    da = torch.zeros(B, H, W, Cn, dtype=dp.dtype, device=dp.device)
    for r in (0, 1):
        for s in (0, 1):
            yv = y[:, r:2 * Hp:2, s:2 * Wp:2, :]
            da[:, r:2 * Hp:2, s:2 * Wp:2, :] = torch.where((idx == r * 2 + s) & (yv > 0), dp, torch.zeros_like(dp))
    return da


def prepare_maxpool2_bwd(it, mem):
    dp_p, idx_p, y_p, da_p, B, H, W, Cn, dtype = it.args
    t = _dt(dtype)
    Hp, Wp = H // 2, W // 2
    dp = mem.view(dp_p, B * Hp * Wp * Cn, t).view(B, Hp, Wp, Cn).clone()
    idx = mem.view(idx_p, B * Hp * Wp * Cn, torch.uint8).view(B, Hp, Wp, Cn).clone()
    y = mem.view(y_p, B * H * W * Cn, t).view(B, H, W, Cn).clone()
    outs = {"da": (mem.view(da_p, B * H * W * Cn, t).view(B, H, W, Cn), True)}
    _poison(outs, [])

    def fn(got):
        exact_bar(got["da"], maxpool2_bwd_expect(dp, idx, y, H, W), f"{it.tag} B{B} {H}x{W} C{Cn}")
        return [(it.tag, f"B{B} {H}x{W} C{Cn}", 0.0)]
    return Check(outs, fn)


def _stem_windows(H, Hp, device):
    """Input rows of the 3x3 / stride-2 / pad-1 windows: [Hp, 3] index (clamped) and validity."""
    iy = torch.arange(Hp, device=device).view(Hp, 1) * 2 - 1 + torch.arange(3, device=device).view(1, 3)
    return iy.clamp(0, H - 1), (iy >= 0) & (iy < H)


def prepare_bn_relu_maxpool(it, mem):
    y_p, sc_p, sh_p, p_p, idx_p, B, H, W, Cn, Hp, Wp, dtype = it.args
    t = _dt(dtype)
    y = mem.view(y_p, B * H * W * Cn, t).view(B, H, W, Cn).clone()
    sc, sh = mem.view(sc_p, Cn, torch.float32).clone(), mem.view(sh_p, Cn, torch.float32).clone()
    outs = {"p": (mem.view(p_p, B * Hp * Wp * Cn, t).view(B, Hp, Wp, Cn), True),
            "idx": (mem.view(idx_p, B * Hp * Wp * Cn, torch.uint8).view(B, Hp, Wp, Cn), True)}
    _poison(outs, [])

    def fn(got):
        a = torch.relu(y.double() * sc.double() + sh.double())              # [B, H, W, C]
        ry, vy = _stem_windows(H, Hp, y.device)
        rx, vx = _stem_windows(W, Wp, y.device)
        # window values [B, Hp, Wp, C, 9] (-inf outside the image), tap k = r * 3 + s
        win = a[:, ry.reshape(-1)][:, :, rx.reshape(-1)].view(B, Hp, 3, Wp, 3, Cn)
        ok = (vy.view(1, Hp, 3, 1, 1, 1) & vx.view(1, 1, 1, Wp, 3, 1))
        win = torch.where(ok, win, torch.full_like(win, float("-inf"))).permute(0, 1, 3, 5, 2, 4).reshape(B, Hp, Wp, Cn, 9)
        mx = win.max(-1).values
        _e, r = tight_ratio(got["p"], mx, 2, f"{it.tag} values", exact_min=0.999)
        k = got["idx"].long()
        assert int(k.max()) <= 8, f"{it.tag}: index byte out of range"
        chosen = win.gather(-1, k.unsqueeze(-1)).squeeze(-1)
        # the chosen tap is a maximum (fp32 ties: within 2^-23 of it) and no EARLIER tap is >= it (the first maximum wins)
        assert bool((chosen >= mx - 2.0 ** -23 * mx.abs()).all()), f"{it.tag}: arg-max index does not point at a maximum"
        pos = torch.arange(9, device=y.device)
        earlier = (pos < k.unsqueeze(-1)) & (win >= chosen.unsqueeze(-1))
        assert not bool(earlier.any()), f"{it.tag}: an earlier tap ties the maximum (first maximum must win)"
        return [(it.tag, f"B{B} {H}x{W} C{Cn} -> {Hp}x{Wp}", r)]
    return Check(outs, fn)


def maxpool_bwd_expect(dp, idx, H, W):
    """da[b, iy, ix] = sum, in the kernel's order (py, then px ascending), over the 3x3 / s2 / p1 windows whose arg-max byte names (iy, ix), of
    dp -- fp32 adds, then one rounding to the storage dtype."""
    B, Hp, Wp, Cn = dp.shape
    dev = dp.device
    iy, ix = torch.arange(H, device=dev), torch.arange(W, device=dev)
    acc = torch.zeros(B, H, W, Cn, dtype=torch.float32, device=dev)
    for jy in (0, 1):
        py = (iy >> 1) + jy * (iy & 1)
        vy = (py <= (iy + 1) >> 1) & (py < Hp) if jy else (py < Hp)
        if jy:
            vy = vy & ((iy & 1) == 1)
        ry = iy - (py * 2 - 1)
        vy = vy & (ry >= 0) & (ry <= 2)
        for jx in (0, 1):
            px = (ix >> 1) + jx * (ix & 1)
            vx = (px < Wp) & (((ix & 1) == 1) if jx else torch.ones_like(px, dtype=torch.bool))
            rx = ix - (px * 2 - 1)
            vx = vx & (rx >= 0) & (rx <= 2)
            g = dp[:, py.clamp(max=Hp - 1)][:, :, px.clamp(max=Wp - 1)].float()
            k = idx[:, py.clamp(max=Hp - 1)][:, :, px.clamp(max=Wp - 1)].long()
            want = (ry.view(H, 1) * 3 + rx.view(1, W)).view(1, H, W, 1)
            hit = (k == want) & vy.view(1, H, 1, 1) & vx.view(1, 1, W, 1)
            acc = acc + torch.where(hit, g, torch.zeros_like(g))
    return acc.to(dp.dtype)


def prepare_maxpool_bwd(it, mem):
    dp_p, idx_p, da_p, B, H, W, Cn, Hp, Wp, dtype = it.args
    t = _dt(dtype)
    dp = mem.view(dp_p, B * Hp * Wp * Cn, t).view(B, Hp, Wp, Cn).clone()
    idx = mem.view(idx_p, B * Hp * Wp * Cn, torch.uint8).view(B, Hp, Wp, Cn).clone()
    outs = {"da": (mem.view(da_p, B * H * W * Cn, t).view(B, H, W, Cn), True)}
    _poison(outs, [])

    def fn(got):
        exact_bar(got["da"], maxpool_bwd_expect(dp, idx, H, W), f"{it.tag} B{B} {H}x{W} C{Cn}")
        return [(it.tag, f"B{B} {Hp}x{Wp} -> {H}x{W} C{Cn}", 0.0)]
    return Check(outs, fn)


def prepare_scatter_stride(it, mem):
    src_p, dx_p, B, H, W, Cn, Ho, Wo, stride, dtype = it.args
    t = _dt(dtype)
    src = mem.view(src_p, B * Ho * Wo * Cn, t).view(B, Ho, Wo, Cn).clone()
    outs = {"dx": (mem.view(dx_p, B * H * W * Cn, t).view(B, H, W, Cn), True)}
    _poison(outs, [])

    def fn(got):
        e = torch.zeros(B, H, W, Cn, dtype=t, device=src.device)
        hh, ww = min(Ho, -(-H // stride)), min(Wo, -(-W // stride))
        e[:, 0:hh * stride:stride, 0:ww * stride:stride] = src[:, :hh, :ww]
        exact_bar(got["dx"], e, f"{it.tag} B{B} {Ho}x{Wo} -> {H}x{W} C{Cn}")
        return [(it.tag, f"B{B} {Ho}x{Wo} -> {H}x{W} C{Cn} s{stride}", 0.0)]
    return Check(outs, fn)


def prepare_im2col(it, mem):
    x_p, A_p, B, Cin, H, W, Ho, Wo, KH, KW, stride, pad, ldk, dtype = it.args
    t = _dt(dtype)
    x = mem.view(x_p, B * Cin * H * W, torch.float32).view(B, Cin, H, W).clone()
    outs = {"A": (mem.view(A_p, B * Ho * Wo * ldk, t).view(B * Ho * Wo, ldk), True)}
    _poison(outs, [])

    def fn(got):
        K = Cin * KH * KW
        A = got["A"]
        for b in range(B):                                          # (one image at a time: the unfolded fp32 matrix stays small)
            u = F.unfold(x[b:b + 1], (KH, KW), padding=pad, stride=stride)[0]       # [K, L], k = ci * KH * KW + r * KW + s
            assert u.shape[1] == Ho * Wo
            exact_bar(A[b * Ho * Wo:(b + 1) * Ho * Wo, :K], u.t().to(t), f"{it.tag} image {b}")
        exact_bar(A[:, K:], torch.zeros_like(A[:, K:]), f"{it.tag}: K padding")
        return [(it.tag, f"B{B} {H}x{W} {KH}x{KW} s{stride} -> M{B * Ho * Wo} K{K} ld{ldk}", 0.0)]
    return Check(outs, fn)


def prepare_colsum(it, mem, wide):
    if wide:
        src_p, out_p, M, ld, Cn, dtype = it.args
        acc = 0
    else:
        src_p, out_p, M, ld, Cn, acc, dtype = it.args
    t = _dt(dtype)
    src = mem.view(src_p, (M - 1) * ld + Cn, t)
    src = torch.as_strided(src, (M, Cn), (ld, 1)).clone()
    out = mem.view(out_p, Cn, torch.float32)
    prev = out.clone() if acc else None
    outs = {"out": (out, not acc)}
    _poison(outs, [])

    def fn(got):
        a = src.double()
        ref = a.sum(0)
        if wide:                       # fp32 partials over row ranges (csrc/bn_pool.hip simt_colsum_wide), combined in double
            rpar = 256 // (Cn // 8)
            rpb = -(-M // 1024)
            rpb = max(rpar, -(-rpb // rpar) * rpar)
            tol = fp32_sum_bound(a.abs(), rpb, ref)
        else:                          # double accumulation throughout, one rounding to fp32
            tol = 2.0 ** -23 * ref.abs() + M * 2.0 ** -50 * a.abs().sum(0)
        if prev is not None:
            ref = ref + prev.double()
            tol = tol + 2.0 ** -23 * ref.abs()
        return [(it.tag, f"M{M} C{Cn}", fp32_bar(got["out"], ref, tol, f"{it.tag} M{M} C{Cn}"))]
    return Check(outs, fn)


def prepare_vec_acc(it, mem):
    dst_p, src_p, n, acc = it.args
    src = mem.view(src_p, n, torch.float32).clone()
    dst = mem.view(dst_p, n, torch.float32)
    prev = dst.clone() if acc else None
    outs = {"dst": (dst, not acc)}
    _poison(outs, [])

    def fn(got):
        exact_bar(got["dst"], prev + src if acc else src, f"{it.tag} n{n}")
        return [(it.tag, f"n{n}{' accumulate' if acc else ''}", 0.0)]
    return Check(outs, fn)


def prepare_bn_fold(it, mem):
    g_p, b_p, rm_p, rv_p, eps, sc_p, sh_p, Cn = it.args
    g, b, rm, rv = (mem.view(p, Cn, torch.float32).clone() for p in (g_p, b_p, rm_p, rv_p))
    outs = {"scale": (mem.view(sc_p, Cn, torch.float32), True), "shift": (mem.view(sh_p, Cn, torch.float32), True)}
    _poison(outs, [])

    def fn(got):
        sc = g.double() / (rv.double() + eps).sqrt()
        sh = b.double() - rm.double() * sc
        r = fp32_bar(got["scale"], sc, 2.0 ** -21 * sc.abs(), "bn_fold scale")
        r = max(r, fp32_bar(got["shift"], sh, 2.0 ** -22 * b.double().abs() + 2.0 ** -20 * (rm.double() * sc).abs(), "bn_fold shift"))
        return [(it.tag, f"C{Cn}", r)]
    return Check(outs, fn)


def prepare_upsample(it, mem):
    src_p, B, h, w, lds, Cn, H, W, align, dst_p = it.args
    src = torch.as_strided(mem.view(src_p, (B * h * w - 1) * lds + Cn, torch.float32), (B, h, w, Cn), (h * w * lds, w * lds, lds, 1)).clone()
    outs = {"dst": (mem.view(dst_p, B * Cn * H * W, torch.float32).view(B, Cn, H, W), True)}
    _poison(outs, [])

    def fn(got):
        s64 = src.double().permute(0, 3, 1, 2)
        ref = F.interpolate(s64, size=(H, W), mode="bilinear", align_corners=bool(align))
        # fp32 source coordinates (dst + 0.5) * h / H - 0.5 carry <= 2 * 2^-24 * max(h, w) absolute error, which moves each of the two weights of
        # an axis by as much: <= 8 * 2^-24 * max(h, w) * max|src| in all; plus four fp32 roundings of the weighted sum
        mx = s64.abs().amax(dim=(2, 3), keepdim=True)
        tol = (8.0 * max(h, w) + 8.0) * U * mx
        return [(it.tag, f"B{B} C{Cn} {h}x{w} -> {H}x{W}", fp32_bar(got["dst"], ref, tol.expand_as(ref), it.tag))]
    return Check(outs, fn)


def prepare_upsample_bwd(it, mem):
    dd_p, B, h, w, lds, Cn, H, W, align, ds_p, dtype, tmp_p = it.args
    t = _dt(dtype)
    ddst = mem.view(dd_p, B * Cn * H * W, torch.float32).view(B, Cn, H, W).clone()
    full = mem.view(ds_p, B * h * w * lds, t).view(B * h * w, lds)
    outs = {"dsrc": (full[:, :Cn], True), "tmp": (mem.view(tmp_p, B * Cn * H * w, torch.float32), True)}
    restore = []
    if Cn < lds:
        restore.append((full[:, Cn:], full[:, Cn:].clone()))
    _poison(outs, [])
    for (pc, _s) in restore:
        pc.fill_(SENTINEL)

    def fn(got):
        for (pc, _s) in restore:
            assert bool((pc == SENTINEL).all()), f"{it.tag}: columns [C, lds) were written"
        s64 = torch.zeros(B, Cn, h, w, dtype=F64, device=ddst.device, requires_grad=True)
        F.interpolate(s64, size=(H, W), mode="bilinear", align_corners=bool(align)).backward(ddst.double())
        ref = s64.grad.permute(0, 2, 3, 1).reshape(B * h * w, Cn)
        # each low-res element sums ~(2H/h + 2) (2W/w + 2) weighted terms in two fp32 passes
        K = (2 * H // h + 2) * (2 * W // w + 2)
        _e, r = tight_bf16_ratio(got["dsrc"], ref, K, f"{it.tag} B{B} C{Cn}") if t == BF else (
            0, fp32_bar(got["dsrc"], ref, 16 * K ** 0.5 * U * ref.pow(2).mean().sqrt().item() + 2.0 ** -22 * ref.abs(), it.tag))
        return [(it.tag, f"B{B} C{Cn} {H}x{W} -> {h}x{w}", r)]
    return Check(outs, fn, restore)


def _tap_args(d):
    return [(int(d.dy[t]), int(d.dx[t])) for t in range(d.ntaps)]


def prepare_tap_gather_sum(it, mem):
    d = it.keep
    M = d.B * d.H * d.W
    P = mem.view(d.src, M * d.lds, torch.float32).view(M, d.lds).clone()
    bias = mem.view(d.bias, d.Q, torch.float32).clone() if d.bias else None
    full = mem.view(d.dst, M * d.ldd, torch.float32).view(M, d.ldd)
    outs = {"dst": (full[:, :d.QP], True)}
    restore = [(full[:, d.QP:], full[:, d.QP:].clone())] if d.QP < d.ldd else []
    _poison(outs, [])
    for (pc, _s) in restore:
        pc.fill_(SENTINEL)

    def fn(got):
        for (pc, _s) in restore:
            assert bool((pc == SENTINEL).all()), f"{it.tag}: columns [QP, ldd) were written"
        m = torch.arange(M, device=P.device)
        oy, ox = (m // d.W) % d.H, m % d.W
        ref = torch.zeros(M, d.QP, dtype=F64, device=P.device)
        absum = torch.zeros_like(ref)
        if bias is not None:
            ref[:, :d.Q] += bias.double()
            absum[:, :d.Q] += bias.double().abs()
        for t, (a, b) in enumerate(_tap_args(d)):
            ok = ((oy + a >= 0) & (oy + a < d.H) & (ox + b >= 0) & (ox + b < d.W)).unsqueeze(1)
            src = (m + a * d.W + b).clamp(0, M - 1)
            v = P[src, t * d.QP:(t + 1) * d.QP].double() * ok
            ref += v
            absum += v.abs()
        tol = (d.ntaps + 1) * U * absum                             # <= ntaps fp32 additions, worst case
        return [(it.tag, f"M{M} taps{d.ntaps} QP{d.QP}", fp32_bar(got["dst"], ref, tol, it.tag))]
    return Check(outs, fn, restore)


def prepare_tap_scatter(it, mem):
    d = it.keep
    M = d.B * d.H * d.W
    src = mem.view(d.src, M * d.lds, BF).view(M, d.lds).clone()
    full = mem.view(d.dst, M * d.ldd, BF).view(M, d.ldd)
    nt = d.ntaps * d.QP
    outs = {"dst": (full[:, :nt], True)}
    restore = [(full[:, nt:], full[:, nt:].clone())] if nt < d.ldd else []
    _poison(outs, [])
    for (pc, _s) in restore:
        pc.fill_(SENTINEL)

    def fn(got):
        for (pc, _s) in restore:
            assert bool((pc == SENTINEL).all()), f"{it.tag}: columns [ntaps * QP, ldd) were written"
        m = torch.arange(M, device=src.device)
        oy, ox = (m // d.W) % d.H, m % d.W
        e = torch.zeros(M, nt, dtype=BF, device=src.device)
        for t, (a, b) in enumerate(_tap_args(d)):
            ok = ((oy - a >= 0) & (oy - a < d.H) & (ox - b >= 0) & (ox - b < d.W)).unsqueeze(1)
            s_ = src[(m - (a * d.W + b)).clamp(0, M - 1), :d.QP]
            e[:, t * d.QP:(t + 1) * d.QP] = torch.where(ok, s_, torch.zeros_like(s_))
        exact_bar(got["dst"], e, it.tag)
        return [(it.tag, f"M{M} taps{d.ntaps} QP{d.QP}", 0.0)]
    return Check(outs, fn, restore)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# direct 7x7 / stride-2 / pad-3 stem (csrc/stem7.hip): packing, forward with up to two weight sets, weight gradient from the image
# ---------------------------------------------------------------------------------------------------------------------------------------------
STEM_TILE = (8, 32)            # output pixels of one statistics slot (simt_stem7_tiles: one slot per 8 x 32 tile)


class _StemGeom:
    """The stem as a conv geometry for conv_rows / conv_gather / wgrad_ref: 49 taps (r - 3, s - 3), stride 2, K = 49 x 3 tap-major."""

    def __init__(self, B, H, W, Ho, Wo):
        self.B, self.H, self.W, self.Ho, self.Wo, self.stride, self.ntaps = B, H, W, Ho, Wo, 2, 49
        self.dy = [r - 3 for r in range(7) for s in range(7)]
        self.dx = [s - 3 for r in range(7) for s in range(7)]


def stem_operand(x_nchw):
    """The image as the stem kernels stage it: each fp32 value rounded once to bf16 (f2bf, round to nearest even), NHWC."""
    return x_nchw.to(BF).permute(0, 2, 3, 1).contiguous()


def stem_tile_sums(v, tiles_shape):
    """v: [B, Ho, Wo, C] float64 -> [tiles, C] sums over each 8 x 32 tile, slot t = (b * tiles_y + ty) * tiles_x + tx (zero-padded edges)."""
    B, Ho, Wo, Cn = v.shape
    ty, tx = tiles_shape
    vp = v.new_zeros(B, ty * STEM_TILE[0], tx * STEM_TILE[1], Cn)
    vp[:, :Ho, :Wo] = v
    return vp.view(B, ty, STEM_TILE[0], tx, STEM_TILE[1], Cn).sum((2, 4)).reshape(B * ty * tx, Cn)


def prepare_stem7_pack(it, mem):
    """dst[o][r][s * 3 + c] = bf16(fp32(w[o][c][r][s] * cscale[o])) (one fp32 product, then f2bf), or bf16(w) without a scale; columns 21..31
    zero.  Bit-exact."""
    w_p, cs_p, dst_p = it.args
    w = mem.view(w_p, 64 * 147, torch.float32).view(64, 3, 7, 7).clone()
    cs = mem.view(cs_p, 64, torch.float32).clone() if cs_p else None
    outs = {"dst": (mem.view(dst_p, 64 * 7 * 32, BF).view(64, 7, 32), True)}
    _poison(outs, [])

    def fn(got):
        v = w.permute(0, 2, 3, 1)                                               # [o][r][s][c]
        if cs is not None:
            v = v * cs.view(64, 1, 1, 1)                                         # fp32 product, rounded once
        e = torch.zeros(64, 7, 32, dtype=BF, device=w.device)
        e[:, :, :21] = v.reshape(64, 7, 21).to(BF)
        exact_bar(got["dst"], e, f"{it.tag}{' (folded scale)' if cs is not None else ''}")
        return [(it.tag, "64 x 7 x 32" + (" (folded scale)" if cs is not None else ""), 0.0)]
    return Check(outs, fn)


def prepare_stem7_fwd(it, mem, seed=0):
    """Every weight set of the launch against float64 on the bf16-rounded image, on conv_rows' sample (every row whose 7x7 window leaves the
    image included).  A set with statistics stores bf16(conv) (one rounding, K = 147 storage bar) and its [tiles][2][64] slots are each held to
    the fp32 blocked-summation bound over the tile's STORED values; a set with bias + ReLU stores bf16(relu(conv + bias)), rounded once."""
    d = it.keep
    B, H, W, Ho, Wo, ns = d.B, d.H, d.W, d.Ho, d.Wo, d.nsets
    M = B * Ho * Wo
    lib = L.load()
    tiles = lib.simt_stem7_tiles(B, Ho, Wo)
    ts = (-(-Ho // STEM_TILE[0]), -(-Wo // STEM_TILE[1]))
    assert tiles == B * ts[0] * ts[1]
    xb = stem_operand(mem.view(d.x, B * 3 * H * W, torch.float32).view(B, 3, H, W))
    reads = [("x", d.x, B * 3 * H * W * 4)]
    outs, sets = {}, []
    for i in range(ns):
        w = mem.view(d.w[i], 64 * 7 * 32, BF).view(64, 7, 32).clone()
        reads.append((f"w{i}", d.w[i], 64 * 7 * 32 * 2))
        bias = mem.view(d.bias[i], 64, torch.float32).clone() if d.bias[i] else None
        outs[f"y{i}"] = (mem.view(d.y[i], M * 64, BF).view(M, 64), True)
        if d.stats[i]:
            outs[f"stats{i}"] = (mem.view(d.stats[i], tiles * 2 * 64, torch.float32).view(tiles, 2, 64), True)
        sets.append((i, w[:, :, :21].reshape(64, 147), bias, int(d.relu[i]), bool(d.stats[i])))   # (order r, s, c = conv_gather's tap-major K)
    _poison(outs, [r[1:] for r in reads])
    g = _StemGeom(B, H, W, Ho, Wo)
    rows = conv_rows(g, xb.device, seed=seed)
    shape = f"M{M} N64 K147 direct 7x7 s2, {ns} set(s)"

    def fn(got):
        recs = []
        inner_all = conv_ref(xb, torch.cat([s_[1] for s_ in sets]), g, rows)            # [S, 64 * nsets]
        for (i, _w, bias, relu, stats) in sets:
            inner = inner_all[:, 64 * i:64 * (i + 1)]
            v = inner + bias.double() if bias is not None else inner
            if relu:
                v = torch.relu(v)
            what = f"{it.tag} set {i}"
            _e, r = tight_bf16_ratio(got[f"y{i}"][rows], v, 147, what)
            recs.append((it.tag + f" [set {i}{' +bias' if bias is not None else ''}{' relu' if relu else ''}]", shape, r))
            if stats:
                yv = got[f"y{i}"].double().view(B, Ho, Wo, 64)
                s1, s2 = stem_tile_sums(yv, ts), stem_tile_sums(yv * yv, ts)
                a1 = stem_tile_sums(yv.abs(), ts)
                R = STEM_TILE[0] * STEM_TILE[1]
                st = got[f"stats{i}"].double()
                rr = max(fp32_bar(st[:, 0], s1, 16.0 * U * R ** 0.5 * a1 + 2.0 ** -22 * s1.abs(), what + " statistics slots (sum)"),
                         fp32_bar(st[:, 1], s2, 16.0 * U * R ** 0.5 * s2 + 2.0 ** -22 * s2, what + " statistics slots (sum of squares)"))
                recs.append((it.tag + f" [set {i} stats, {tiles} slots]", shape, rr))
        return recs
    return Check(outs, fn, reads=reads)


def stem7_wgrad_reduce_expect(part):
    """dW from the workgroups' partials [nwg][64][7][32] in the documented fixed order (csrc/stem7.hip stem7_wgrad_reduce_kernel): row q of 16
    adds partials q, q + 16, ... in order, then the 16 row sums are added in order -- fp32 adds, bit for bit -- mapped k' = s * 3 + c to OIHW."""
    nwg = part.shape[0]
    p2 = part.reshape(nwg, -1)
    rows = []
    for q in range(16):
        t = torch.zeros_like(p2[0])
        for g_ in range(q, nwg, 16):
            t = t + p2[g_]
        rows.append(t)
    v = rows[0]
    for q in range(1, 16):
        v = v + rows[q]
    return v.view(64, 7, 32)[:, :, :21].reshape(64, 7, 7, 3).permute(0, 3, 1, 2).contiguous()


def prepare_stem7_wgrad(it, mem):
    """dw [64][3][7][7] against float64 conv2d_weight(bf16(image), dy) with the fp32 blocked-summation bound of the weight-gradient bar's form
    (blocks = the persistent workgroups' pixel sets, then <= 256 partials added in fp32); the workspace `part` is poisoned too and must be
    written whole, and dw must be its fixed-order sum (stem7_wgrad_reduce_expect) bit for bit."""
    x_p, dy_p, part_p, dw_p, B, H, W, Ho, Wo = it.args[:9]
    lib = L.load()
    nwg = lib.simt_stem7_wgrad_workgroups(B, Ho, Wo)
    M = B * Ho * Wo
    xb = stem_operand(mem.view(x_p, B * 3 * H * W, torch.float32).view(B, 3, H, W))
    dy = mem.view(dy_p, M * 64, BF).view(M, 64).clone()
    reads = [("x", x_p, B * 3 * H * W * 4), ("dy", dy_p, M * 64 * 2)]
    outs = {"part": (mem.view(part_p, nwg * 64 * 7 * 32, torch.float32).view(nwg, 64, 7, 32), True),
            "dw": (mem.view(dw_p, 64 * 147, torch.float32).view(64, 3, 7, 7), True)}
    _poison(outs, [r[1:] for r in reads])
    g = _StemGeom(B, H, W, Ho, Wo)
    shape = f"M{M} direct, {nwg} workgroups"

    def fn(got):
        # float64 reference and the per-workgroup absolute sums: tile t = (b * tiles_y + ty) * tiles_x + tx goes to workgroup t % nwg
        dev = dy.device
        m = torch.arange(M, device=dev)
        ty_n, tx_n = -(-Ho // STEM_TILE[0]), -(-Wo // STEM_TILE[1])
        t = ((m // (Ho * Wo)) * ty_n + ((m // Wo) % Ho) // STEM_TILE[0]) * tx_n + (m % Wo) // STEM_TILE[1]
        wg = t % nwg
        order = torch.argsort(wg, stable=True)
        counts = torch.bincount(wg, minlength=nwg).tolist()
        ref = torch.zeros(64, 147, dtype=F64, device=dev)
        a2 = torch.zeros(64, 147, dtype=F64, device=dev)
        GEMM_FLOPS[0] += 4.0 * M * 64 * 147
        off, step = 0, 16
        for g0 in range(0, nwg, step):
            n = sum(counts[g0:g0 + step])
            rows = order[off:off + n]
            X = conv_gather(xb, g, rows)                                       # [n, 147] float64, (r, s, c)
            D = dy[rows].double()
            o2 = 0
            for c in counts[g0:g0 + step]:
                Dg, Xg = D[o2:o2 + c], X[o2:o2 + c]
                ref += Dg.t() @ Xg
                a2 += (Dg.abs().t() @ Xg.abs()).pow(2)
                o2 += c
            off += n
        R = max(counts)
        ref4 = ref.view(64, 7, 7, 3).permute(0, 3, 1, 2)
        tol = (16.0 * U * (R ** 0.5 + nwg ** 0.5) * a2.sqrt()).view(64, 7, 7, 3).permute(0, 3, 1, 2) + 2.0 ** -22 * ref4.abs()
        r = fp32_bar(got["dw"], ref4, tol, f"{it.tag} dw vs float64")
        assert not bool(torch.isnan(got["part"]).any()), f"{it.tag}: workspace partials not written whole"
        exact_bar(got["dw"], stem7_wgrad_reduce_expect(got["part"]), f"{it.tag}: dw vs the fixed-order sum of the partials")
        return [(it.tag, shape, r)]
    return Check(outs, fn, reads=reads, problems=[("dy", "x", "dw")])


# ---------------------------------------------------------------------------------------------------------------------------------------------
def fn_name(it):
    return getattr(it.fn, "__name__", None)


def prepare(it, mem, ctx):
    """Check for launch `it`, or None if no handler covers its C entry point.  ctx: dict(pack_jobs=[...], dst_sizes=callable) for the packs.
    Every range the handler viewed that is neither an output nor a named read is added to chk.reads as in{k}."""
    h = HANDLERS.get(fn_name(it))
    if h is None:
        return None
    mem.log = []
    try:
        chk = h(it, mem, ctx)
    finally:
        log, mem.log = mem.log, None
    known = {extent(v) for (v, _p) in chk.outs.values()} | {(p, n) for (_k, p, n) in chk.reads}
    for (p, n) in log:
        if (p, n) not in known:
            chk.reads.append((f"in{len(chk.reads)}", p, n))
            known.add((p, n))
    return chk


def _pack_multi(it, mem, ctx):
    import numpy as np
    jobs_t, _ch = it.keep
    raw = jobs_t.cpu().numpy().view(np.dtype([("w", "<u8"), ("dst", "<u8"), ("cscale", "<u8"), ("ldk", "<i8"), ("total", "<i8"),
                                              ("Cout", "<i4"), ("Cin", "<i4"), ("RS", "<i4"), ("row_off", "<i4"), ("tap_off", "<i4"),
                                              ("Ck", "<i4"), ("mode", "<i4"), ("dtype", "<i4")]))
    jobs = [(int(j["w"]), int(j["dst"]), int(j["cscale"]), int(j["ldk"]), int(j["Cout"]), int(j["Cin"]), int(j["RS"]), int(j["row_off"]),
             int(j["tap_off"]), int(j["Ck"]), int(j["mode"]), int(j["dtype"])) for j in raw]
    return prepare_pack(it, mem, jobs, ctx["dst_sizes"])


def _pack_one(it, mem, ctx):
    w, dst, cout, cin, rs, row_off, tap_off, ldk, ck, mode, cscale, dtype = it.args
    return prepare_pack(it, mem, [(w, dst, cscale or 0, ldk, cout, cin, rs, row_off, tap_off, ck, mode, dtype)], ctx["dst_sizes"])


def _wgrad_multi(it, mem, ctx):
    _table, descs, _slabs = it.keep
    return prepare_wgrad_descs(it, descs, mem)


def _reduce_multi(it, mem, ctx):
    _rt, rjobs = it.keep
    return prepare_wgrad_reduce(it, mem, [(j["slab"].data_ptr(), j["dst"].data_ptr(), j["nsplit"], j["Cd"], j["Ktot"], j["Cin"], j["co_off"],
                                           j["tap_off"], j["Cout"], j["RS"], int(j.get("accumulate", False))) for j in rjobs])


HANDLERS = {
    "simt_conv_fprop": lambda it, mem, ctx: prepare_conv(it, mem, seed=ctx.get("seed", 0)),
    "simt_conv_wgrad": lambda it, mem, ctx: prepare_wgrad_descs(it, [it.keep], mem),
    "simt_conv_wgrad_multi": _wgrad_multi,
    "simt_wgrad_reduce": lambda it, mem, ctx: prepare_wgrad_reduce(it, mem, [tuple(it.args)]),
    "simt_wgrad_reduce_multi": _reduce_multi,
    "simt_wgrad_reduce_exp": lambda it, mem, ctx: prepare_wgrad_reduce_exp(it, mem),
    "simt_pack_weight": _pack_one,
    "simt_pack_weight_multi": _pack_multi,
    "simt_bn_fold": lambda it, mem, ctx: prepare_bn_fold(it, mem),
    "simt_bn_finalize": lambda it, mem, ctx: prepare_bn_finalize(it, mem),
    "simt_bn_apply": lambda it, mem, ctx: prepare_bn_apply(it, mem, False),
    "simt_bn_apply_bits": lambda it, mem, ctx: prepare_bn_apply(it, mem, True),
    "simt_bn_bwd": lambda it, mem, ctx: prepare_bn_bwd(it, mem),
    "simt_maxpool2": lambda it, mem, ctx: prepare_maxpool2(it, mem),
    "simt_maxpool2_bwd": lambda it, mem, ctx: prepare_maxpool2_bwd(it, mem),
    "simt_bn_relu_maxpool": lambda it, mem, ctx: prepare_bn_relu_maxpool(it, mem),
    "simt_maxpool_bwd": lambda it, mem, ctx: prepare_maxpool_bwd(it, mem),
    "simt_scatter_stride": lambda it, mem, ctx: prepare_scatter_stride(it, mem),
    "simt_im2col_stem": lambda it, mem, ctx: prepare_im2col(it, mem),
    "simt_colsum": lambda it, mem, ctx: prepare_colsum(it, mem, False),
    "simt_colsum_wide": lambda it, mem, ctx: prepare_colsum(it, mem, True),
    "simt_vec_acc": lambda it, mem, ctx: prepare_vec_acc(it, mem),
    "simt_upsample_nchw": lambda it, mem, ctx: prepare_upsample(it, mem),
    "simt_upsample_nchw_bwd": lambda it, mem, ctx: prepare_upsample_bwd(it, mem),
    "simt_tap_gather_sum": lambda it, mem, ctx: prepare_tap_gather_sum(it, mem),
    "simt_tap_scatter": lambda it, mem, ctx: prepare_tap_scatter(it, mem),
    "simt_stem7_pack": lambda it, mem, ctx: prepare_stem7_pack(it, mem),
    "simt_stem7_fwd": lambda it, mem, ctx: prepare_stem7_fwd(it, mem, seed=ctx.get("seed", 0)),
    "simt_stem7_wgrad": lambda it, mem, ctx: prepare_stem7_wgrad(it, mem),
}
