"""The early optimiser step of SimTTrainer as a checked property (step.py `_backward_early_sgd`).  Not collected (no test_ prefix).

The schedule: the backward launch list is replayed up to item `cut`; an event is recorded on the main stream; the side stream waits for it
(it is in-order, so it also holds every side-stream launch before the cut), then runs SGD and the re-pack of the applied parameters, while
the main stream replays the items from `cut` on.  Side-stream items from `cut` on queue BEHIND SGD and the re-pack.

Pure bookkeeping over byte ranges (`check_cut`, no torch, no GPU: tests/test_step_hazards_cpu.py runs it on synthetic lists).  Reported:

  war          a main-stream launch at or after the cut READS a range SGD or the re-pack writes: it may see the new or the old bytes
  side-reads   a side-stream launch at or after the cut reads such a range: it runs behind SGD, so it sees the NEW bytes where the plain
               schedule (SGD after the backward) shows it the old ones
  late-grad    a launch at or after the cut, on either stream, WRITES an applied gradient: SGD reads it too early (main stream) or has
               already read it (side stream)
  no-writer    an applied gradient that no launch before the cut writes

`plan_launches` (GPU) turns a plan's real backward list into the `Launch` records: tests/_launch_oracle.prepare for every entry that has a
handler, the descriptors themselves for conv launches that carry a fused BatchNorm (which the oracle refuses)."""
from collections import namedtuple

Launch = namedtuple("Launch", "index name stream reads writes")      # reads / writes: [(label, address, bytes)]
Violation = namedtuple("Violation", "kind index name what")


def overlap(a, b):
    """(label, address, bytes) ranges; empty ranges overlap nothing."""
    return a[2] > 0 and b[2] > 0 and a[1] < b[1] + b[2] and b[1] < a[1] + a[2]


def check_cut(launches, cut, sgd_reads, sgd_writes, pack_writes):
    """launches: Launch records in list order, `index` = position in the backward list (events / waits are simply absent).  cut: SGD and the
    re-pack are enqueued on the side stream once items [0, cut) are enqueued.  sgd_reads: the applied gradients; sgd_writes: applied masters
    and momentum buffers; pack_writes: destinations of the re-pack.  -> [Violation]."""
    out = []
    side_writes = list(sgd_writes) + list(pack_writes)
    for l in launches:
        if l.index < cut:
            continue
        for r in l.reads:
            for w in side_writes:
                if overlap(r, w):
                    out.append(Violation("war" if l.stream == 0 else "side-reads", l.index, l.name,
                                         f"reads {r[0]} which overlaps {w[0]} written by the early optimiser step"))
        for w in l.writes:
            for g in sgd_reads:
                if overlap(w, g):
                    out.append(Violation("late-grad", l.index, l.name, f"writes {w[0]} which overlaps the applied gradient {g[0]}"))
    for g in sgd_reads:
        if not any(overlap(w, g) for l in launches if l.index < cut for w in l.writes):
            out.append(Violation("no-writer", -1, "", f"applied gradient {g[0]} has no writer before the cut"))
    return out


def earlier_cut(cut, hook_points):
    """The hook point before `cut` (hook points: the distinct values of plan.grad_ready), or None."""
    before = [c for c in sorted(set(hook_points)) if c < cut]
    return before[-1] if before else None


# ---------------------------------------------------------------------------------------------------------------------------------------------
# real plans (GPU)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def conv_desc_ranges(d):
    """Reads and writes of a simt_conv_fprop launch from its descriptors alone (simt_conv_desc + simt_fbn_desc hold every pointer and
    extent): used where the launch carries a fused BatchNorm.  Extents are whole pitched buffers (never smaller than what is touched)."""
    import ctypes as C

    from simt_amd import _lib as L
    esz_in = 2 if d.dtype_in == L.SIMT_BF16 else 4
    esz_out = 2 if d.dtype_out == L.SIMT_BF16 else 4
    M, K = d.B * d.Ho * d.Wo, d.ntaps * d.Cin
    reads = [("x", d.x, d.B * d.H * d.W * d.Cin * esz_in), ("w", d.w, d.Npad * K * esz_in)]
    writes = [("y", d.y, M * d.ldy * esz_out)]
    if d.bias:
        reads.append(("bias", d.bias, d.Cout * 4))
    if d.res:
        reads.append(("res", d.res, M * d.ldr * esz_in))
    if d.res_bits:
        reads.append(("res_bits", d.res_bits, M * d.ldr // 8))
    if d.mask:
        reads.append(("mask", d.mask, M * d.ldm * esz_in))
    if d.in_scale:
        reads += [("in_scale", d.in_scale, d.Cin * 4), ("in_shift", d.in_shift, d.Cin * 4)]
        writes.append(("in_out", d.in_out, d.B * d.H * d.W * d.Cin * esz_in))
    if d.bnr_mode:
        reads += [("bnr_y", d.bnr_y, M * d.bnr_ld * esz_in), ("bnr_mean", d.bnr_mean, d.Cout * 4), ("bnr_rstd", d.bnr_rstd, d.Cout * 4)]
        if d.bnr_mode == 2:
            reads += [("bnr_scale", d.bnr_scale, d.Cout * 4), ("bnr_shift", d.bnr_shift, d.Cout * 4)]
        else:
            reads.append(("bnr_bits", d.bnr_bits, M * d.Cout // 8))
        writes.append(("bnr_part", d.bnr_part, max(1, L.load().simt_conv_mtiles(C.byref(d))) * 3 * d.Cout * 4))
    if d.stats:
        writes.append(("stats", d.stats, -(-M // 128) * 2 * d.Cout * 4))
    if d.fbn:
        f = d._fbn_keep
        writes += [("fbn.out", f.out, M * f.ldo * esz_out), ("fbn.work", f.work, L.load().simt_conv_fbn_words(C.byref(d)) * 8),
                   ("fbn.err", f.err, 8)]
        reads.append(("fbn.work", f.work, L.load().simt_conv_fbn_words(C.byref(d)) * 8))
        if f.mode == 1:
            reads += [("fbn.gamma", f.gamma, d.Cout * 4), ("fbn.beta", f.beta, d.Cout * 4)]
            writes += [(f"fbn.{k}", getattr(f, k), d.Cout * 4) for k in ("running_mean", "running_var", "mean", "rstd", "scale", "shift")]
        else:
            writes.append(("fbn.coef", f.coef, 3 * d.Cout * 4))
            reads.append(("fbn.coef", f.coef, 3 * d.Cout * 4))
            if f.dgamma:
                writes += [("fbn.dgamma", f.dgamma, d.Cout * 4), ("fbn.dbeta", f.dbeta, d.Cout * 4)]
    return reads, writes


def plan_launches(plan, lst, others=()):
    """Launch records of the list `lst` of `plan` with their real byte ranges.  NOTE: the oracle's prepare poisons the outputs of the
    launches it handles; build the plan for this purpose only.  -> (launches, unhandled tags)."""
    import _launch_oracle as lo
    import _plan_replay as pr
    mem = pr._mem(plan, *others)
    ctx = {"seed": 0, "dst_sizes": lambda ptr, dt: (sum(mem.span_of(ptr)) - ptr) // (2 if dt == lo.BF else 4)}
    out, unhandled = [], []
    for i, it in enumerate(lst.items):
        if it.fn is None:
            continue
        name = lo.fn_name(it)
        if name == "simt_conv_fprop" and it.keep.fbn:
            reads, writes = conv_desc_ranges(it.keep)
        else:
            chk = lo.prepare(it, mem, ctx)
            if chk is None:
                unhandled.append(f"{i} {name} <{it.tag}>")
                continue
            reads, writes = list(chk.reads), chk.writes()
            chk.finish()
            del chk
        out.append(Launch(i, f"{name} <{it.tag}>", it.stream, reads, writes))
    return out, unhandled


def trainer_ranges(tr):
    """(sgd_reads, sgd_writes, pack_writes) of a SimTTrainer: applied gradients, applied masters + momentum buffers, and the destinations of
    the subset re-pack (whole destination buffers: the pack writes into them at offsets)."""
    import _launch_oracle as lo
    import _plan_replay as pr
    mem = pr._mem(tr.plan)
    nb = lambda t: t.numel() * t.element_size()
    sgd_reads = [(n, tr.plan.grads[n].data_ptr(), nb(tr.plan.grads[n])) for n in tr.sgd_names]
    sgd_writes = [(n, tr.params[n].data_ptr(), nb(tr.params[n])) for n in tr.sgd_names]
    sgd_writes += [(n + " (momentum)", tr.mom[n].data_ptr(), nb(tr.mom[n])) for n in tr.sgd_names]
    names = {t.data_ptr(): n for n, t in tr.plan.p.items()}
    applied = {tr.params[n].data_ptr() for n in tr.sgd_names}
    pack_writes = []
    for it in tr.plan._pack_items_raw:
        fn = lo.fn_name(it)
        if fn == "simt_pack_weight":
            if it.args[0] not in applied:
                continue
            start, nbytes = mem.span_of(it.args[1])
            pack_writes.append((f"{names[it.args[0]]} ({'dgrad' if (it.args[9] & 0xFF) == 1 else 'fprop'} operand)", start, nbytes))
        elif fn == "simt_vec_acc":
            pack_writes.append((f"bias sum <- {names.get(it.args[1], hex(it.args[1]))}", it.args[0], 4 * it.args[2]))
        elif fn == "simt_bn_fold":
            pack_writes += [("BatchNorm fold scale", it.args[5], 4 * it.args[7]), ("BatchNorm fold shift", it.args[6], 4 * it.args[7])]
        elif fn == "simt_stem7_pack":
            pack_writes.append(("stem pack", it.args[2], 64 * 7 * 32 * 2))
    return sgd_reads, sgd_writes, pack_writes
