"""Launch-by-launch replay of a plan's LaunchLists under the float64 oracle (tests/_launch_oracle.py), shared by tests/test_gpu_plan_launches.py
(DeepLabv3, DeepLab-VGG16) and tests/test_gpu_plan_launches_v2.py (DeepLab-v2).  Not collected (no test_ prefix).

Every launch is replayed ONE AT A TIME on one stream, its inputs snapshotted and its outputs poisoned before it runs, and checked right after;
the chain then continues on the kernel's own result.  A launch without a handler is recorded as uncovered.  Optionally every launch's reads
and writes feed a last-writer trace (tests/_plan_trace.py)."""
import torch

import _launch_oracle as lo
from simt_amd import _lib as L


def _key(d):
    return (d.B, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout, d.stride, tuple(lo.conv_taps_of(d)))


def _k(Bn, Hi, Wi, Cin, Ho, Wo, Cout, stride, taps):
    return (Bn, Hi, Wi, Cin, Ho, Wo, Cout, stride, tuple(taps))


def _neg(taps):
    return [(-a, -b) for (a, b) in taps]


STEM_TAPS = [(r - 3, s - 3) for r in range(7) for s in range(7)]


def stem_key(d):
    """Geometry of the direct stem launch (simt_stem_desc) in _key's form: Cin 3, Cout 64, stride 2, the 49 taps of a 7x7 window at pad 3."""
    return _k(d.B, d.H, d.W, 3, d.Ho, d.Wo, 64, 2, STEM_TAPS)


def match_layers(plan, run, layers, train):
    """Each recorded conv launch -> the parameter(s) packed into the buffer its weight operand points into (the plan's pack jobs), in the packing
    direction (mode 1 = dgrad operand); its geometry must be that layer's.  Records which (layer, direction) pairs were launched.  The direct
    stem's packer (simt_stem7_pack) counts as conv1.weight's forward packing."""
    mem = _mem(plan)
    names = {t.data_ptr(): n[:-len(".weight")] for n, t in plan.p.items() if n.endswith(".weight")}
    packs = {}
    for it in plan._pack_items_raw:
        if lo.fn_name(it) == "simt_stem7_pack":
            packs.setdefault(mem.span_of(it.args[2])[0], set()).add((names[it.args[0]], "fwd"))
            continue
        if lo.fn_name(it) != "simt_pack_weight":
            continue
        w, dst, mode = it.args[0], it.args[1], it.args[9]
        packs.setdefault(mem.span_of(dst)[0], set()).add((names[w], "bwd" if (mode & 0xFF) == 1 else "fwd"))
    for (where, dirn, key, wptr) in run.convs:
        owners = packs.get(mem.span_of(wptr)[0])
        if not owners:
            run.layer_bad.append(f"{where}: weight operand not packed from any parameter")
            continue
        for (pname, pdir) in sorted(owners):
            want = layers.get(pname, {}).get(pdir)
            if pdir != dirn or want != key:
                run.layer_bad.append(f"{where}: operand packed from {pname} ({pdir}) expects {want}, launch has {key} ({dirn})")
            else:
                run.layer_seen.add((pname, pdir))
    want_all = {(n, dd) for n, g in layers.items() for dd in (("fwd", "bwd") if train else ("fwd",)) if g[dd] is not None}
    run.layer_missing = sorted(want_all - run.layer_seen)


def _mem(plan, *others):
    """Every tensor the plan (and the partner plans `others`: a frozen plan whose stem runs in the trainable plan's launch) owns."""
    ts = []
    for pl in (plan,) + tuple(others):
        ts += list(pl._keep) + list(pl._bufs.values()) + list(pl.p.values())
        if getattr(pl, "flat_grad", None) is not None:
            ts.append(pl.flat_grad)
        for lst in (pl.pack_list, pl.fwd_list, pl.bwd_list):
            for it in lst.items:
                if isinstance(it.keep, tuple):
                    ts += [t for t in it.keep if isinstance(t, torch.Tensor)]
    return lo.Mem(ts)


class Run:
    def __init__(self):
        self.worst = {}          # (tag, shape) -> worst error / bound
        self.fail, self.uncovered = [], []
        self.convs = []          # (where, "fwd" | "bwd", geometry, weight operand pointer) of every conv launch
        self.layer_bad, self.layer_seen, self.layer_missing = [], set(), []
        self.secs, self.tflop = 0.0, 0.0
        self.red = {}            # what -> list of perturbations the checker caught
        self.n = 0


def replay(plan, lists, run, red=None, seed=0, others=(), trace=None, not_here=()):
    """Replay the lists item by item under the oracle.  red(lname, it, chk, got): optional hook called after a green check.  others: partner
    plans whose buffers the lists also touch.  trace: a _plan_trace.Tracer fed with every prepared launch's reads and writes.  not_here: tags
    held by other tests (an unhandled launch with such a tag is not reported as uncovered)."""
    mem = _mem(plan, *others)
    stream = torch.cuda.current_stream().cuda_stream
    ctx = {"seed": seed, "dst_sizes": lambda ptr, dt: (sum(mem.span_of(ptr)) - ptr) // torch.empty((), dtype=dt).element_size()}
    for lname, lst in lists:
        for i, it in enumerate(lst.items):
            if it.fn is None:
                continue
            name = lo.fn_name(it)
            where = f"{lname}[{i}] {name} <{it.tag}> {it.shape or ''}"
            if name == "simt_conv_fprop":
                assert not it.keep.fbn, f"{where}: fused BatchNorm launch although SIMT_BN_GRID=0"
                run.convs.append((where, "bwd" if lname.endswith("bwd") else "fwd", _key(it.keep), it.keep.w))
            elif name == "simt_stem7_fwd":
                for s in range(it.keep.nsets):
                    run.convs.append((f"{where} set {s}", "fwd", stem_key(it.keep), it.keep.w[s]))
            try:
                chk = lo.prepare(it, mem, ctx)
            except (AssertionError, KeyError, NotImplementedError) as e:
                run.fail.append(f"{where}: cannot prepare: {e}")
                chk = None
            if chk is None and lo.HANDLERS.get(name) is None and it.tag not in not_here:
                run.uncovered.append(where)
            if trace is not None and chk is not None:
                trace.launch(lname, i, name, it.tag, chk.reads, chk.writes(), chk.problems, chk.jobs)
            rc = it.fn(*it.args, stream)
            if rc != 0:
                L.check(rc)
            if chk is None:
                continue
            torch.cuda.synchronize()
            got = chk.outputs()
            try:
                for (tag, shape, r) in chk.check(got):
                    key = (tag, shape)
                    run.worst[key] = max(run.worst.get(key, 0.0), r)
                if red is not None:
                    red(lname, it, chk, got)
            except (AssertionError, NotImplementedError, RuntimeError) as e:
                run.fail.append(f"{where}: {e}")
            chk.finish()
            run.n += 1
            del chk, got


def _env(mp):
    mp.setenv("SIMT_SINGLE_STREAM", "1")
    mp.setenv("SIMT_BN_GRID", "0")
    import simt_amd.engine as eng
    eng._SIDE_STREAMS.clear()


def _perturb(chk, got, what, cases):
    """Each case: (name, mutate(copy of got)) -> the checker must raise AssertionError."""
    caught = []
    for name, mut in cases:
        g2 = {k: v.clone() for k, v in got.items()}
        mut(g2)
        try:
            chk.check(g2)
        except AssertionError:
            caught.append(name)
    return caught


def _two_ulps(t, idx):
    v = t[idx].double()
    t[idx] = (v + 2.5 * lo.ulp_bf16(v.abs(), 1e-30) * (1 if v >= 0 else -1)).to(t.dtype)
