"""tests/_step_hazards.check_cut on synthetic launch lists: a clean early optimiser step, and one list per violation it must report
(write-after-read on a re-packed operand, on a master, a side-stream reader of updated bytes, a late gradient writer on either stream, an
applied gradient nobody wrote before the cut).  No GPU."""
import _step_hazards as sh
from _step_hazards import Launch

# a toy address map (bytes): gradients, masters, momentum, packed operands, activations
G = {"l4.w": ("grad l4.w", 0x1000, 256), "l3.w": ("grad l3.w", 0x1100, 256), "l2.w": ("grad l2.w", 0x1200, 256)}
P = {"l4.w": ("l4.w", 0x2000, 256), "l3.w": ("l3.w", 0x2100, 256), "l2.w": ("l2.w", 0x2200, 256)}
MOM = {"l4.w": ("l4.w (momentum)", 0x3000, 256), "l3.w": ("l3.w (momentum)", 0x3100, 256)}
WT = {"l4.w": ("l4.w (dgrad operand)", 0x4000, 128), "l3.w": ("l3.w (dgrad operand)", 0x4100, 128), "l2.w": ("l2.w (dgrad operand)", 0x4200, 128)}
ACT = [("dy%d" % i, 0x8000 + 0x100 * i, 256) for i in range(8)]
APPLIED = ["l4.w", "l3.w"]
SGD_READS = [G[n] for n in APPLIED]
SGD_WRITES = [P[n] for n in APPLIED] + [MOM[n] for n in APPLIED]
PACK_WRITES = [WT[n] for n in APPLIED]


def clean():
    """dgrad chain on the main stream (0), weight gradients on the side stream (1); the applied gradients are final at item 6."""
    return [
        Launch(0, "dgrad l4", 0, [ACT[0], WT["l4.w"]], [ACT[1]]),
        Launch(2, "wgrad l4", 1, [ACT[0], ACT[7]], [G["l4.w"]]),
        Launch(3, "dgrad l3", 0, [ACT[1], WT["l3.w"]], [ACT[2]]),
        Launch(5, "wgrad l3", 1, [ACT[1], ACT[7]], [G["l3.w"]]),
        Launch(6, "dgrad l2", 0, [ACT[2], WT["l2.w"]], [ACT[3]]),
        Launch(8, "wgrad l2", 1, [ACT[2], ACT[7]], [G["l2.w"]]),
    ]


def kinds(v):
    return sorted({x.kind for x in v})


def test_clean_list_has_no_violation():
    assert sh.check_cut(clean(), 6, SGD_READS, SGD_WRITES, PACK_WRITES) == []
    assert sh.check_cut(clean(), 8, SGD_READS, SGD_WRITES, PACK_WRITES) == []          # a later cut is safe too, only slower


def test_cut_one_hook_point_early_is_reported():
    """Cut before the dgrad that reads l3's packed operand and before l3's weight gradient: a write-after-read, a late writer, and an applied
    gradient without a writer before the cut."""
    cut = sh.earlier_cut(6, [3, 6, 9])
    assert cut == 3 and sh.earlier_cut(3, [3, 6, 9]) is None
    v = sh.check_cut(clean(), cut, SGD_READS, SGD_WRITES, PACK_WRITES)
    assert kinds(v) == ["late-grad", "no-writer", "war"]
    assert [x.what for x in v if x.kind == "no-writer"] == ["applied gradient grad l3.w has no writer before the cut"]
    war = [x for x in v if x.kind == "war"]
    assert len(war) == 1 and war[0].index == 3 and "l3.w (dgrad operand)" in war[0].what
    late = [x for x in v if x.kind == "late-grad"]
    assert len(late) == 1 and late[0].index == 5 and "grad l3.w" in late[0].what


def test_main_stream_reader_of_a_repacked_operand_after_the_cut():
    ls = clean()
    ls[4] = Launch(6, "dgrad l2 (shortcut through l3's operand)", 0, [ACT[2], WT["l2.w"], ("tail of l3's operand", 0x4100 + 127, 1)], [ACT[3]])
    v = sh.check_cut(ls, 6, SGD_READS, SGD_WRITES, PACK_WRITES)
    assert [x.kind for x in v] == ["war"] and v[0].index == 6 and "l3.w (dgrad operand)" in v[0].what
    ls[4] = Launch(6, "dgrad l2", 0, [ACT[2], WT["l2.w"], ("the byte behind l3's operand", 0x4100 + 128, 1)], [ACT[3]])
    assert sh.check_cut(ls, 6, SGD_READS, SGD_WRITES, PACK_WRITES) == []


def test_main_stream_reader_of_a_master_or_momentum_after_the_cut():
    for rng in (P["l4.w"], MOM["l3.w"]):
        ls = clean() + [Launch(9, "late reader", 0, [rng], [ACT[4]])]
        v = sh.check_cut(ls, 6, SGD_READS, SGD_WRITES, PACK_WRITES)
        assert [x.kind for x in v] == ["war"] and v[0].index == 9 and rng[0] in v[0].what


def test_side_stream_reader_after_the_cut_sees_updated_bytes():
    ls = clean() + [Launch(9, "side reader", 1, [WT["l4.w"]], [ACT[4]])]
    v = sh.check_cut(ls, 6, SGD_READS, SGD_WRITES, PACK_WRITES)
    assert [x.kind for x in v] == ["side-reads"] and v[0].index == 9


def test_late_writer_of_an_applied_gradient_on_either_stream():
    for stream in (0, 1):
        ls = clean() + [Launch(9, "second writer", stream, [ACT[3]], [("half of grad l4.w", 0x1000 + 128, 128)])]
        v = sh.check_cut(ls, 6, SGD_READS, SGD_WRITES, PACK_WRITES)
        assert [x.kind for x in v] == ["late-grad"] and v[0].index == 9 and "grad l4.w" in v[0].what


def test_applied_gradient_without_a_writer_before_the_cut():
    ls = [l for l in clean() if l.name != "wgrad l4"]
    v = sh.check_cut(ls, 6, SGD_READS, SGD_WRITES, PACK_WRITES)
    assert [x.kind for x in v] == ["no-writer"] and "grad l4.w" in v[0].what
    # unapplied gradients may be written whenever: l2's weight gradient after the cut is no violation (clean list), and it needs no writer
    assert sh.check_cut([l for l in clean() if l.name != "wgrad l2"], 6, SGD_READS, SGD_WRITES, PACK_WRITES) == []


def test_empty_ranges_overlap_nothing():
    assert not sh.overlap(("a", 0x10, 0), ("b", 0x10, 16)) and sh.overlap(("a", 0x10, 1), ("b", 0x10, 16))
    assert not sh.overlap(("a", 0x10, 16), ("b", 0x20, 16)) and sh.overlap(("a", 0x10, 17), ("b", 0x20, 16))
