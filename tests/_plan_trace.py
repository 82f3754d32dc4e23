"""Last-writer trace of a plan replay, and the operand rules checked on it (pure Python: tests/test_plan_trace_cpu.py runs it on the CPU).

The float64 oracle (tests/_launch_oracle.py) checks each launch against whatever its pointers hold when it runs.  That cannot see a launch
that computes the right answer for the WRONG input -- a weight gradient reading a dY buffer set another Bottleneck has already overwritten,
or a BatchNorm backward reading a saved activation a backward launch has reused.  The trace keeps, per byte range of device memory, the launch
that wrote it last; every replayed launch records the last writers of the ranges it reads at the moment it runs.  Memory present before the
replay has the writer INIT; the test's own writes (the image, the seeded dlogits) are writers of phase "test".

    tr = Tracer(block_of)                      # block_of(lname, index) -> Bottleneck name or None (messages only)
    tr.write("test", 0, "image", addr, nbytes)
    tr.launch(lname, index, fn, tag, reads, writes, problems, jobs)     # reads / writes: [(name, addr, nbytes)]
    violations = check_rules(tr, grads, dy_window, fwd, bwd, x_from_test)
"""
import bisect
from collections import namedtuple

Writer = namedtuple("Writer", "lname index tag block out")
INIT = Writer("init", -1, "init", None, None)


class IntervalMap:
    """Disjoint half-open byte intervals [lo, hi) -> value; the gaps map to INIT."""

    def __init__(self):
        self.lo, self.hi, self.val = [], [], []

    def _span(self, lo, hi):
        # intervals overlapping [lo, hi): the first whose end is > lo up to the last whose start is < hi (both lists are sorted)
        return bisect.bisect_right(self.hi, lo), bisect.bisect_left(self.lo, hi)

    def assign(self, lo, hi, v):
        if hi <= lo:
            return
        i, j = self._span(lo, hi)
        new = []
        if i < j and self.lo[i] < lo:
            new.append((self.lo[i], lo, self.val[i]))
        new.append((lo, hi, v))
        if i < j and self.hi[j - 1] > hi:
            new.append((hi, self.hi[j - 1], self.val[j - 1]))
        self.lo[i:j] = [a for a, _b, _v in new]
        self.hi[i:j] = [b for _a, b, _v in new]
        self.val[i:j] = [w for _a, _b, w in new]

    def query(self, lo, hi):
        """[(lo, hi, value)] covering [lo, hi) in address order, gaps as INIT."""
        out, pos = [], lo
        i, j = self._span(lo, hi)
        for k in range(i, j):
            a, b = max(self.lo[k], lo), min(self.hi[k], hi)
            if a > pos:
                out.append((pos, a, INIT))
            out.append((a, b, self.val[k]))
            pos = b
        if pos < hi:
            out.append((pos, hi, INIT))
        return out


class Launch:
    """One traced launch: src = {read name: [(lo, hi, Writer)]} as it was when the launch ran; writes = [(name, lo, hi)];
    problems = [(dy read, x read, output)] (weight gradients); jobs = [(slab read, destination output)] (slab reduces)."""
    __slots__ = ("lname", "index", "fn", "tag", "block", "src", "writes", "problems", "jobs")

    def __init__(self, lname, index, fn, tag, block, src, writes, problems, jobs):
        self.lname, self.index, self.fn, self.tag, self.block = lname, index, fn, tag, block
        self.src, self.writes, self.problems, self.jobs = src, writes, list(problems), list(jobs)

    def where(self):
        return f"{self.lname}[{self.index}] {self.fn} <{self.tag}>{' ' + self.block if self.block else ''}"


class Tracer:
    def __init__(self, block_of=None):
        self.map = IntervalMap()
        self.launches = []
        self.by_key = {}
        self.block_of = block_of or (lambda lname, index: None)

    def write(self, lname, index, tag, lo, nbytes, out="test"):
        """A write outside the launch lists (the test's copy of the image / of dlogits)."""
        self.map.assign(lo, lo + nbytes, Writer(lname, index, tag, None, out))

    def launch(self, lname, index, fn, tag, reads, writes, problems=(), jobs=()):
        block = self.block_of(lname, index)
        src = {name: self.map.query(lo, lo + n) for (name, lo, n) in reads}
        rec = Launch(lname, index, fn, tag, block, src, [(name, lo, lo + n) for (name, lo, n) in writes], problems, jobs)
        for (name, lo, hi) in rec.writes:
            self.map.assign(lo, hi, Writer(lname, index, tag, block, name))
        self.launches.append(rec)
        self.by_key[(lname, index)] = rec
        return rec


CONV_FNS = ("simt_conv_fprop", "simt_stem7_fwd")
WGRAD_FNS = ("simt_conv_wgrad", "simt_conv_wgrad_multi", "simt_stem7_wgrad")
BN_BWD_FNS = ("simt_bn_bwd",)


def _act_reads(rec):
    """The activation operands R1 holds: conv x / res, weight-gradient dy / x, BatchNorm-backward dz / y."""
    if rec.fn in CONV_FNS:
        return [n for n in rec.src if n in ("x", "res")]
    if rec.fn in WGRAD_FNS:
        return [n for n in rec.src if n in ("x", "dy") or (n[:2] == "dy" and n[2:].isdigit()) or (n[:1] == "x" and n[1:].isdigit())]
    if rec.fn in BN_BWD_FNS:
        return [n for n in rec.src if n in ("dz", "y")]
    return []


def _fmt(w):
    return "init (before the replay)" if w is INIT else f"{w.lname}[{w.index}] <{w.tag}>{' ' + w.block if w.block else ''} ({w.out})"


def check_rules(tr, grads, dy_window, fwd, bwd, x_from_test=()):
    """Violations of R1-R3 (strings; empty = the trace holds).

    grads: {address of a weight gradient tensor: parameter name}; dy_window: {parameter name: (lo, hi)} -- the indices of the backward list
    `bwd` within which the parameter's dY must have been written (its Bottleneck's backward range; the stem: after layer1.0's; a head: its
    own part of the list); fwd: the name of the trainable forward list; x_from_test: parameters whose x is the test's image.
      R1  no activation operand of a conv, weight gradient or BatchNorm backward (any list) was last written by INIT;
      R2  every weight-gradient problem is traced to its parameter (problem -> slab -> the reduce job writing grads[name], or written into
          grads[name] directly): its dY was last written inside dy_window[name] of `bwd`, its x in `fwd` (or by the test's image copy for
          x_from_test); every parameter of `grads` is reached;
      R3  the y / bnr_y (and y2, z) operands of the trainable plan's BatchNorm backwards and fused reduces were last written in `fwd`; the dz
          operands of its BatchNorm backwards in `bwd`."""
    bad = []
    for rec in tr.launches:
        for n in _act_reads(rec):
            if any(w is INIT for (_a, _b, w) in rec.src[n]):
                bad.append(f"R1: {rec.where()}: operand {n} was last written by nobody in the replay (init)")

    def r2(param, wrec, prob, via):
        dyn, xn, _out = prob
        lo, hi = dy_window[param]
        for (_a, _b, w) in wrec.src[dyn]:
            if not (w.lname == bwd and lo <= w.index < hi):
                bad.append(f"R2: {param} ({via}{wrec.where()}): dY operand {dyn} last written by {_fmt(w)}, not inside {bwd}[{lo}:{hi}]")
        for (_a, _b, w) in wrec.src[xn]:
            if not (w.lname == fwd or (param in x_from_test and w.lname == "test")):
                bad.append(f"R2: {param} ({via}{wrec.where()}): x operand {xn} last written by {_fmt(w)}, not by the forward list {fwd}")

    reached, used = set(), set()
    for rec in tr.launches:
        outs = {name: (lo, hi) for (name, lo, hi) in rec.writes}
        for prob in rec.problems:                          # weight gradients written straight into a parameter's gradient (the stem)
            lo = outs[prob[2]][0]
            if lo in grads:
                reached.add(grads[lo])
                used.add((rec.lname, rec.index, prob[2]))
                if grads[lo] in dy_window:
                    r2(grads[lo], rec, prob, "")
                else:
                    bad.append(f"R2: {rec.where()}: no dY window for {grads[lo]}")
        for (slab, dst) in rec.jobs:
            lo = outs[dst][0]
            if lo not in grads:
                continue
            param = grads[lo]
            ws = {w for (_a, _b, w) in rec.src[slab]}
            if len(ws) != 1 or next(iter(ws)) is INIT:
                bad.append(f"R2: {param} ({rec.where()}): slab {slab} not written by one weight-gradient problem: {sorted(_fmt(w) for w in ws)}")
                continue
            w = next(iter(ws))
            wrec = tr.by_key.get((w.lname, w.index))
            prob = [p for p in (wrec.problems if wrec else []) if p[2] == w.out]
            if not prob:
                bad.append(f"R2: {param} ({rec.where()}): slab {slab} last written by {_fmt(w)}, which is no weight-gradient problem")
                continue
            reached.add(param)
            used.add((w.lname, w.index, w.out))
            if param not in dy_window:
                bad.append(f"R2: {rec.where()}: no dY window for {param}")
                continue
            r2(param, wrec, prob[0], f"reduced by {rec.where()} from ")
    missing = sorted(set(grads.values()) - reached)
    if missing:
        bad.append(f"R2: {len(missing)} weight gradient(s) never traced to a weight-gradient problem: {missing[:6]}")
    for rec in tr.launches:
        if rec.lname == bwd:
            for prob in rec.problems:
                if (rec.lname, rec.index, prob[2]) not in used:
                    bad.append(f"R2: {rec.where()}: problem {prob[2]} reaches no parameter's gradient")
    for rec in tr.launches:
        if rec.lname != bwd:
            continue
        saved = [n for n in ("y", "y2", "z") if rec.fn in BN_BWD_FNS and n in rec.src] + [n for n in ("bnr_y", "bnr_bits") if n in rec.src]
        for n in saved:
            for (_a, _b, w) in rec.src[n]:
                if w.lname != fwd:
                    bad.append(f"R3: {rec.where()}: saved operand {n} last written by {_fmt(w)}, not by the forward list {fwd}")
        if rec.fn in BN_BWD_FNS:
            for (_a, _b, w) in rec.src["dz"]:
                if w.lname != bwd:
                    bad.append(f"R3: {rec.where()}: dz last written by {_fmt(w)}, not by the backward list {bwd}")
    return bad
