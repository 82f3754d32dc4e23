"""The last-writer trace and its operand rules (tests/_plan_trace.py) on synthetic launch records: a correct trace passes, and each kind of
wrong operand the rules exist for is reported under its rule.  No GPU."""
import random

from _plan_trace import INIT, IntervalMap, Tracer, check_rules

GRADS = {10_000: "A.conv.weight", 11_000: "B.conv.weight"}
WINDOW = {"A.conv.weight": (0, 5), "B.conv.weight": (5, 10)}


def _trace(other_block_dy=False, bwd_overwrites_x=False, bwd_overwrites_y=False, init_read=False):
    """Two Bottlenecks A, B over the same buffers: forward (conv -> BatchNorm apply), then each block's backward (dgrad conv -> BatchNorm
    backward -> weight gradient -> slab reduce into its parameter's gradient).  Addresses in bytes; each buffer 100 bytes."""
    tr = Tracer()
    tr.write("test", 0, "image", 0, 100)
    tr.launch("fwd", 0, "simt_conv_fprop", "conv", [("x", 0, 100), ("w", 5000, 100)], [("y", 100, 100)])
    tr.launch("fwd", 1, "simt_bn_apply", "bn", [("in0", 100, 100)], [("z", 200, 100)])
    tr.launch("fwd", 2, "simt_conv_fprop", "conv", [("x", 200, 100), ("w", 5100, 100)], [("y", 300, 100)])
    tr.write("test", 0, "dlogits", 400, 100)
    for blk, base, y, x, grad in (("A", 0, 300, 200, 10_000), ("B", 5, 100, 200, 11_000)):
        bwd = [(base + 0, "simt_conv_fprop", [("x", 400, 100), ("w", 5200, 100)], [("y", 500, 100)], (), ()),
               (base + 1, "simt_bn_bwd", [("dz", 500, 100), ("y", y, 100)], [("dy", 600, 100), ("coef", 7000, 16)], (), ()),
               (base + 3, "simt_conv_wgrad_multi", [("dy0", 600, 100), ("x0", x, 100)], [("slab0", 8000, 100)], [("dy0", "x0", "slab0")], ()),
               (base + 4, "simt_wgrad_reduce_multi", [("slab0", 8000, 100)], [("dst0", grad, 40)], (), [("slab0", "dst0")])]
        for (i, fn, reads, writes, probs, jobs) in bwd:
            if blk == "B" and fn == "simt_conv_wgrad_multi" and other_block_dy:
                # B's weight gradient reads the dY buffer set block A's backward (index 2 of ITS range) overwrote: wrong buffer rotation
                tr.launch("bwd", 2, "simt_bn_bwd", "bn_bwd", [("dz", 500, 100), ("y", 300, 100)], [("dy", 600, 100)])
            if blk == "B" and fn == "simt_conv_wgrad_multi" and bwd_overwrites_x:
                tr.launch("bwd", 7, "simt_scatter_stride", "scatter", [("in0", 500, 100)], [("dx", 200, 100)])
            if blk == "B" and fn == "simt_bn_bwd" and bwd_overwrites_y:
                tr.launch("bwd", 6, "simt_scatter_stride", "scatter", [("in0", 500, 100)], [("dx", 100, 100)])
            if init_read and fn == "simt_conv_fprop" and blk == "B":
                reads = [("x", 9000, 100), ("w", 5200, 100)]
            tr.launch("bwd", i, fn, fn, reads, writes, probs, jobs)
    return tr


def _rules(tr):
    return check_rules(tr, GRADS, WINDOW, fwd="fwd", bwd="bwd")


def test_correct_trace_passes():
    assert _rules(_trace()) == []


def test_dy_from_another_bottleneck_fails_r2():
    bad = _rules(_trace(other_block_dy=True))
    assert bad and all(b.startswith("R2") for b in bad), bad
    assert any("B.conv.weight" in b and "dY operand" in b for b in bad), bad


def test_saved_activation_overwritten_in_backward_fails():
    bad = _rules(_trace(bwd_overwrites_x=True))
    assert any(b.startswith("R2") and "x operand" in b and "B.conv.weight" in b for b in bad), bad
    bad = _rules(_trace(bwd_overwrites_y=True))
    assert any(b.startswith("R3") and "saved operand y" in b for b in bad), bad


def test_init_read_fails_r1():
    bad = _rules(_trace(init_read=True))
    assert any(b.startswith("R1") and "operand x" in b for b in bad), bad


def test_unreached_gradient_and_unconsumed_problem_fail_r2():
    tr = _trace()
    tr.launch("bwd", 9, "simt_conv_wgrad", "wgrad", [("dy0", 600, 100), ("x0", 0, 100)], [("slab0", 8500, 100)], [("dy0", "x0", "slab0")])
    g = dict(GRADS)
    g[12_000] = "C.conv.weight"
    bad = check_rules(tr, g, WINDOW, fwd="fwd", bwd="bwd")
    assert any("never traced" in b and "C.conv.weight" in b for b in bad), bad
    assert any("reaches no parameter" in b for b in bad), bad


def test_interval_map_matches_a_byte_array():
    """Random assignments against a byte-per-address model: query returns the last writer of every byte, gaps as INIT."""
    rnd = random.Random(3)
    n = 400
    model = [INIT] * n
    m = IntervalMap()
    for k in range(600):
        lo = rnd.randrange(n)
        hi = min(n, lo + rnd.randrange(1, 60))
        m.assign(lo, hi, k)
        model[lo:hi] = [k] * (hi - lo)
        a = rnd.randrange(n)
        b = min(n, a + rnd.randrange(1, 120))
        got = [None] * (b - a)
        pos = a
        for (s, e, v) in m.query(a, b):
            assert s == pos and e > s
            got[s - a:e - a] = [v] * (e - s)
            pos = e
        assert pos == b and got == model[a:b]
    assert all(m.lo[i] < m.hi[i] <= m.lo[i + 1] for i in range(len(m.lo) - 1))
