"""Operand coherence: after an optimiser step, is everything the next forward / backward reads derived from the CURRENT fp32 masters?
Shared by tests/test_gpu_step_coherence.py.  Not collected (no test_ prefix).

A plan derives its operands from the masters through its pack list (`plan._pack_items_raw`): simt_pack_weight in every layout mode (fprop,
dgrad, tap-expanded head; with or without the fragment flag), simt_stem7_pack, simt_bn_fold, simt_vec_acc.  The pack KERNELS are held exactly
by the launch oracle (tests/_launch_oracle.py prepare_pack & co.), so a FRESH plan of the same class and arguments, built from a clone of the
masters (its constructor runs the whole pack list), is an independent reference for FRESHNESS: a plan is coherent when the destination of
every pack-list entry holds, bit for bit, what the fresh plan's entry at the same position wrote.  Both plans add their entries in the same
order, so destinations pair up by position (checked: same entry point, same geometry arguments).

An update too small to change a bf16 rounding cannot show a stale bf16 operand.  `seed_momentum` makes the next SGD step move every applied
element by about 2^-5 relative, and `rounding_changed` measures, from the fp32 masters alone, the fraction of elements whose bf16 rounding
changed; the tests require >= 0.99 for every applied weight tensor (a cap below which a case is vacuous, not a measurement)."""
import numpy as np
import torch

import _launch_oracle as lo
import _plan_replay as pr
from simt_amd.engine import HeadCfg, LaunchList, TrunkPlan

SEG_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("buf", "<u8"), ("n", "<i8"), ("mult", "<i4"), ("group", "<i4")])
MODE_NAMES = {0: "fprop operand", 1: "dgrad operand", 2: "tap-expanded head operand"}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# fresh plans
# ---------------------------------------------------------------------------------------------------------------------------------------------
def device_state(state, dev):
    return {k: v.detach().to(dev, torch.float32 if v.dtype != torch.long else torch.long).clone() for k, v in state.items()}


def fresh_plan(plan, params):
    """A new plan of `plan`'s class and constructor arguments over `params` (device tensors the caller owns).  Must be called under the
    environment the original was built in (SIMT_BN_GRID & co. are read by the constructor)."""
    from simt_amd.engine_v3 import V3Plan
    from simt_amd.engine_vgg import VggPlan
    kw = dict(dtype=plan.dtype, train=plan.train, data_parallel=plan.data_parallel)
    if isinstance(plan, V3Plan):
        return V3Plan(params, plan.B, plan.H, plan.W, plan.nc, plan.openc, plan.openset, layers=plan.v3_layers, width=plan.width,
                      assp_ch=plan.assp_ch, **kw)
    if isinstance(plan, VggPlan):
        return VggPlan(params, plan.B, plan.H, plan.W, plan.heads[0].Q, vgg_layers=plan.vgg_layers, **kw)
    assert type(plan) is TrunkPlan
    heads = [HeadCfg(h.name, h.feat_layer, h.cin, list(h.groups), tuple(h.dilations)) for h in plan.heads]
    assert plan.stem_from is None, "a plan that joins another plan's stem launch is compared against a snapshot, not rebuilt"
    return TrunkPlan(params, plan.B, plan.H, plan.W, heads, layers=plan.layers, grads_from_layer=plan.grads_from_layer, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the pack list of a plan: what each entry writes
# ---------------------------------------------------------------------------------------------------------------------------------------------
class Entry:
    """One pack-list entry: `label` names the source parameter and the packing direction; `source` the parameter name(s) it reads;
    `sig` its non-pointer arguments; `dsts` = [(address, bytes, element positions or None)] it writes."""
    __slots__ = ("fn", "label", "sources", "sig", "dsts")

    def __init__(self, fn, label, sources, sig, dsts):
        self.fn, self.label, self.sources, self.sig, self.dsts = fn, label, sources, sig, dsts


def pack_entries(plan, mem=None):
    mem = mem or pr._mem(plan)
    names = {t.data_ptr(): n for n, t in plan.p.items()}
    dev = plan.dev
    out = []
    for it in plan._pack_items_raw:
        fn = lo.fn_name(it)
        if fn == "simt_pack_weight":
            w, dst, cout, cin, rs, row_off, tap_off, ldk, ck, mode, cscale, dtype = it.args
            esz = 2 if lo._dt(dtype) == lo.BF else 4
            start, nbytes = mem.span_of(dst)
            frag = mode >> 8
            label = f"{names[w]} ({MODE_NAMES[mode & 0xFF]}{', fragment order' if frag else ''}{', BatchNorm scale folded' if cscale else ''})"
            if frag:            # fragment order permutes the whole buffer: compare it whole
                dsts = [(start, nbytes, None, esz)]
            else:
                row, kcol = lo.pack_positions(cout, cin, rs, row_off, tap_off, ldk, ck, mode, dev)
                dsts = [(dst, start + nbytes - dst, (row * ldk + kcol).reshape(-1), esz)]
            out.append(Entry(fn, label, [names[w]], (cout, cin, rs, row_off, tap_off, ldk, ck, mode, bool(cscale), dtype), dsts))
        elif fn == "simt_stem7_pack":
            w, cs, dst = it.args
            out.append(Entry(fn, f"{names[w]} (stem pack{', BatchNorm scale folded' if cs else ''})", [names[w]], (bool(cs),),
                             [(dst, 64 * 7 * 32 * 2, None, 2)]))
        elif fn == "simt_bn_fold":
            g_p, b_p, rm_p, rv_p, eps, sc_p, sh_p, Cn = it.args
            bn = names[g_p][:-len(".weight")]
            out.append(Entry(fn, f"{bn} (BatchNorm fold: scale, shift)", [names[p] for p in (g_p, b_p, rm_p, rv_p)], (eps, Cn),
                             [(sc_p, 4 * Cn, None, 4), (sh_p, 4 * Cn, None, 4)]))
        elif fn == "simt_vec_acc":
            dst, src, n, acc = it.args
            out.append(Entry(fn, f"{names.get(src, hex(src))} (summed bias{', accumulated' if acc else ''})", [names[src]] if src in names else [],
                             (n, acc), [(dst, 4 * n, None, 4)]))
        else:
            raise AssertionError(f"pack list entry {fn} is not known to the coherence check: teach it what the entry writes")
    return out


def _bits(mem, addr, nbytes, pos, esz):
    v = mem.view(addr, nbytes // esz, torch.int16 if esz == 2 else torch.int32)
    return v if pos is None else v[pos]


def snapshot(plan):
    """Bit copies of every pack-list destination of `plan`, entry by entry."""
    mem = pr._mem(plan)
    return [[_bits(mem, a, nb, pos, esz).clone() for (a, nb, pos, esz) in e.dsts] for e in pack_entries(plan, mem)]


def compare(plan, ref, what):
    """Mismatches between `plan`'s pack-list destinations and `ref` -- another plan (paired by position) or a snapshot() of this one.
    -> ["<parameter> (<direction>): k of n elements differ ..."]."""
    mem = pr._mem(plan)
    ents = pack_entries(plan, mem)
    if isinstance(ref, list):
        theirs = ref
        assert len(theirs) == len(ents)
    else:
        rmem = pr._mem(ref)
        rents = pack_entries(ref, rmem)
        assert [(e.fn, e.label, e.sig) for e in ents] == [(e.fn, e.label, e.sig) for e in rents], "the two plans' pack lists do not pair up"
        theirs = [[_bits(rmem, a, nb, pos, esz) for (a, nb, pos, esz) in e.dsts] for e in rents]
    bad = []
    for e, rd in zip(ents, theirs):
        for (a, nb, pos, esz), r in zip(e.dsts, rd):
            mine = _bits(mem, a, nb, pos, esz)
            ndiff = int((mine != r).sum())
            if ndiff:
                bad.append(f"{e.label}: {ndiff} of {mine.numel()} elements differ from {what}")
    return bad, ents


def check_coherent(plan, fresh, applied=None, before=None):
    """-> list of mismatches (empty = coherent).  fresh: a fresh_plan over a clone of the current masters.  applied / before: the names the
    optimiser applies and a snapshot() taken before the step -- every entry none of whose sources is applied must be bit-identical to it."""
    bad, ents = compare(plan, fresh, "a fresh pack of the current masters (STALE)")
    if before is not None:
        mem = pr._mem(plan)
        app = set(applied)
        for e, rd in zip(ents, before):
            if any(s in app for s in e.sources):
                continue
            for (a, nb, pos, esz), r in zip(e.dsts, rd):
                if not torch.equal(_bits(mem, a, nb, pos, esz), r):
                    bad.append(f"{e.label}: changed by a step that does not apply it")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------------------
# a visible update
# ---------------------------------------------------------------------------------------------------------------------------------------------
def sgd_groups(tr):
    """{parameter name: (lr group, multiplicity)} from the trainer's device-side segment table."""
    segs = np.frombuffer(tr.sgd_segs.cpu().numpy().tobytes(), dtype=SEG_DT)
    by_ptr = {int(s["p"]): (int(s["group"]), int(s["mult"])) for s in segs}
    return {n: by_ptr[tr.params[n].data_ptr()] for n in tr.sgd_names}


def seed_momentum(tr, lr, seed):
    """Momentum buffers such that lr_group * momentum * buf = r * 2^-5 * p, r a seeded random sign per element: the next SGD step (first_step
    must be 0: it_done >= 1) moves every applied element by ~2^-5 relative per listing, far more than the gradient term."""
    assert tr.it_done >= 1 and tr.hp.momentum > 0
    g = torch.Generator().manual_seed(seed)
    for n, (group, _mult) in sgd_groups(tr).items():
        p = tr.params[n]
        r = (torch.randint(0, 2, p.shape, generator=g).float() * 2 - 1).to(p.device)
        tr.mom[n].copy_(r * (2.0 ** -5) * p / ((lr * (10.0 if group == 1 else 1.0)) * tr.hp.momentum))


def masters(tr):
    return {n: tr.params[n].detach().cpu().clone() for n in tr.sgd_names}


def rounding_changed(before, after):
    """{name: fraction of elements with bf16(after) != bf16(before)}, on the host, from the fp32 masters alone."""
    bits = lambda t: t.to(torch.bfloat16).view(torch.int16)
    return {n: float((bits(before[n]) != bits(after[n])).double().mean()) for n in before}


def assert_visible(fr, what, cap=0.99):
    """The condition: every applied WEIGHT tensor moved in bf16 on >= cap of its elements (biases may be exactly zero: reported only)."""
    weights = {n: f for n, f in fr.items() if n.endswith(".weight")}
    lo_n = min(weights, key=weights.get)
    print(f"{what}: bf16 rounding changed on >= {weights[lo_n]:.4f} of the elements of each of {len(weights)} applied weight tensors "
          f"(lowest: {lo_n}); other applied tensors: lowest {min([f for n, f in fr.items() if n not in weights], default=float('nan')):.4f}")
    for n, f in sorted(weights.items()):
        print(f"    {n}: {f:.4f}")
    low = {n: f for n, f in weights.items() if f < cap}
    assert not low, f"{what}: vacuous -- the update does not change the bf16 rounding of >= {cap} of the elements of {low}"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# checkpoint round trip
# ---------------------------------------------------------------------------------------------------------------------------------------------
def step_lists(plan):
    """The forward / backward lists the trainers replay: DeepLabv3's in-model upsample and its adjoint are fused into the head kernel."""
    f, b = LaunchList(), LaunchList()
    f.items = [it for it in plan.fwd_list.items if it.tag != "simt_upsample_nchw"]
    b.items = [it for it in plan.bwd_list.items if it.tag != "simt_upsample_nchw_bwd"]
    return f, b


def seed_dlogits(plan, seed=8):
    g = torch.Generator().manual_seed(seed)
    qs = {h.name: h.Q for h in plan.heads}
    for name in sorted(plan.dlogits):
        dl = plan.dlogits[name]
        Q = qs.get(name, getattr(plan, "Q", None))
        dl.zero_()
        dl[:, :Q] = (torch.randn(dl.shape[0], Q, generator=g) * 1e-3).to(dl.dtype).to(dl.device)


def logits_of(plan):
    outs = dict(plan.out)
    if getattr(plan, "logits", None) is not None:
        outs["logits"] = plan.logits
    assert outs
    return outs


def forward_backward(plan, image):
    """One forward and one backward of `plan` on `image` under seeded upstream gradients.  -> {what: clone} of every head's logits, the flat
    gradient and the BatchNorm running statistics."""
    f, b = step_lists(plan)
    plan.x_in.copy_(image)
    f.run()
    seed_dlogits(plan)
    b.run()
    torch.cuda.synchronize()
    res = {f"logits {k}": v.clone() for k, v in logits_of(plan).items()}
    res["flat_grad"] = plan.flat_grad.clone()
    for k, v in plan.p.items():
        if k.endswith(("running_mean", "running_var")):
            res[k] = v.clone()
    return res


def round_trip_mismatches(a, b):
    assert a.keys() == b.keys()
    bad = []
    for k in a:
        x, y = a[k], b[k]
        if not torch.isfinite(x.float()).all():
            bad.append(f"{k}: not finite")
        elif not torch.equal(x, y):
            bad.append(f"{k}: {int((x != y).sum())} of {x.numel()} elements differ between the running trainer and a plan built from its state_dict()")
    return bad
