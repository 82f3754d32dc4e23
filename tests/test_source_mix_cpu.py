"""The labelled source batch without a GPU: the numpy restatement of `simt_source_mix` (tests/_source_mix_ref.py) held to
tests/_class_mix_ref.py on the concatenated 2B-item batch, the descriptor against the header, the signatures, the keyword's checks,
`GTA5DataSet`, the flag of trainV1_warmup and its refusals, the run identity and the train state on fake trainers."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _class_mix_ref as cref
import _source_mix_ref as sref
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd import online_labels as ol
from simt_amd import train_state as tsf
from test_ema_cpu import _advanced, _Fake, _refused, no_device_sync  # noqa: F401  (the fixture is used by name)
from test_online_labels_cb_cpu import _layout
from test_online_weighted_cpu import _FakeWeighted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "simt_hip.h")).read()
CD = so.load_class_dist()
NEW = ["simt_source_mix", "simt_source_mix_items", "simt_head_loss_weighted_n", "simt_head_grad_weighted_n"]


# ---- the restatement against the in-batch ClassMix on the concatenated batch --------------------------------------------------------------------------
def batch(B, h, w, Cn, seed, one_class=None):
    """-> (xs, labs, xt, lab8): int32 words with NaN payloads and -0.0 among them, blocky source labels with 255s and out-of-range values, blocky
    target bytes.  one_class = i: source item i holds ONE class (and nothing else)."""
    g = np.random.default_rng(seed)
    xs = g.integers(-2 ** 31, 2 ** 31, (B, 3, h, w), dtype=np.int64).astype(np.int32)
    xt = g.integers(-2 ** 31, 2 ** 31, (B, 3, h, w), dtype=np.int64).astype(np.int32)
    xs.reshape(-1)[:4] = np.array([0x7FC01234, -0x00345678, -2 ** 31, 0x7F800001], dtype=np.int64).astype(np.int32)      # NaN payloads, -0.0
    xt.reshape(-1)[:4] = np.array([0x7FA0BEEF, -2 ** 31, 0x7FFFFFFF, -0x003FFFFF], dtype=np.int64).astype(np.int32)
    bh, bw = (h + 2) // 3, (w + 4) // 5
    labs = np.repeat(np.repeat(g.integers(0, Cn, (B, bh, bw)), 3, 1), 5, 2)[:, :h, :w].astype(np.int64)
    lab8 = np.repeat(np.repeat(g.integers(0, Cn, (B, (h + 4) // 5, (w + 2) // 3)), 5, 1), 3, 2)[:, :h, :w].astype(np.uint8)
    labs[:, h // 2, :] = 255
    labs[0, 0, 0], labs[-1, -1, -1], labs[0, -1, 0] = Cn, -1, 300
    lab8[:, :, w // 2] = 255
    if one_class is not None:
        labs[one_class] = Cn - 1
    return xs, labs, xt, lab8


def concatenated(xs, labs, xt, lab8, apply, rank, Cn):
    """tests/_class_mix_ref.py on [xt; xs], [widened lab8; labs] with partner[i] = B + i: -> (x_out, lab_out, item map) of the first B items.
    `_class_mix_ref.mix` pairs i with (i + 1) % n, so its masks are taken item by item through `chosen`, its selection through numpy."""
    B = labs.shape[0]
    x2 = np.concatenate([xt, xs])
    lab2 = np.concatenate([lab8.astype(np.int64), labs])
    apply2 = np.concatenate([np.asarray(apply, bool), np.zeros(B, bool)])
    rank2 = np.concatenate([rank, rank])
    partner = [B + i for i in range(B)] + list(range(B, 2 * B))
    m = np.zeros(lab2.shape, bool)
    for i in range(2 * B):
        if apply2[i]:
            j = partner[i]
            S = cref.chosen(lab2[j], rank2[i], Cn)
            m[i] = (lab2[j] >= 0) & (lab2[j] < Cn) & np.isin(lab2[j], sorted(S))
    x_out = np.where(m[:, None], x2[partner], x2)
    lab_out = np.where(m, lab2[partner], lab2)
    own = np.arange(2 * B).reshape(-1, 1, 1)
    item = np.where(m, np.asarray(partner).reshape(-1, 1, 1), own).astype(np.uint8)
    return x_out[:B], lab_out[:B], item[:B]


@pytest.mark.parametrize("B,h,w,Cn,seed", [(2, 33, 37, 19, 1), (3, 16, 64, 19, 2), (1, 8, 8, 5, 3), (16, 12, 20, 32, 4)])
def test_restatement_equals_class_mix_on_the_concatenated_batch(B, h, w, Cn, seed):
    xs, labs, xt, lab8 = batch(B, h, w, Cn, seed, one_class=B - 1)
    for how in ("mixed", "all", "none"):
        apply, rank = cref.draws(cref.generator(seed, 0), B, Cn, 0.5)
        apply = {"none": np.zeros(B, bool), "all": np.ones(B, bool), "mixed": apply}[how]
        got = sref.mix(xs, labs, xt, lab8, apply, rank, Cn)
        want = concatenated(xs, labs, xt, lab8, apply, rank, Cn)
        for a, b, name in zip(got, want, ("x_out", "lab_out", "item")):
            assert a.dtype == b.dtype and np.array_equal(a, b), (how, name)
        m = sref.paste_masks(labs, apply, rank, Cn)
        assert not m[(labs < 0) | (labs >= Cn)].any(), "a 255 or an out-of-range source label was pasted"
        if how == "none":
            assert np.array_equal(got[0], xt) and np.array_equal(got[1], lab8.astype(np.int64))
            assert np.array_equal(got[2], np.broadcast_to(np.arange(B, dtype=np.uint8).reshape(B, 1, 1), labs.shape))
        if how == "all":      # the one-class item pastes its class: k = (1 + 1) // 2 = 1
            assert np.array_equal(m[B - 1], labs[B - 1] == Cn - 1) and m[B - 1].all()


def test_restatement_on_a_hand_made_item():
    labs = np.array([[[0, 0, 1, 2], [2, 3, 255, 7]]], dtype=np.int64)          # C = 4: present {0, 1, 2, 3}, k = 2
    lab8 = np.full((1, 2, 4), 9, dtype=np.uint8)
    xs, xt = np.full((1, 3, 2, 4), 1, np.int32), np.full((1, 3, 2, 4), 2, np.int32)
    rank = np.array([[3, 0, 2, 1]], dtype=np.uint8)                             # smallest ranks: class 1, then class 3
    x, lab, item = sref.mix(xs, labs, xt, lab8, [True], rank, 4)
    assert lab.tolist() == [[[9, 9, 1, 9], [9, 3, 9, 9]]] and item.tolist() == [[[0, 0, 1, 0], [0, 1, 0, 0]]]
    assert x[0, 2].tolist() == [[2, 2, 1, 2], [2, 1, 2, 2]]


# ---- header and descriptors -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_symbols_and_the_descriptor_matches_ctypes():
    assert re.search(r"int simt_source_mix\(const simt_source_mix_desc\* d, simt_stream_t stream\);", HDR)
    assert re.search(r"int simt_source_mix_items\(const simt_source_mix_desc\* d, uint8_t\* item_out, simt_stream_t stream\);", HDR)
    for name in ("simt_head_loss_weighted_n", "simt_head_grad_weighted_n"):
        assert re.search(rf"int {name}\(const simt_head_desc\* d, const float\* w, int nw, const uint8_t\* w_item, simt_stream_t stream\);", HDR)
    assert L.ABI_VERSION == 2 and int(re.search(r"#define\s+SIMT_ABI_VERSION\s+(\d+)", HDR).group(1)) == 2
    assert L.HEAD_WEIGHTS_MAX == 64 == int(re.search(r"#define SIMT_HEAD_WEIGHTS_MAX (\d+)", HDR).group(1)) == 2 * L.CLASS_MIX_MAX
    names = ["xs", "labs", "part_s", "xt", "lab8", "x_out", "lab_out", "B", "h", "w", "n_classes", "apply", "rank"]
    assert [n for n, _t in L.SourceMixDesc._fields_] == names
    out = _layout("simt_source_mix_desc", names)
    assert C.sizeof(L.SourceMixDesc) == out["size"] == 56 + 16 + 32 + 1024
    for n in names:
        assert getattr(L.SourceMixDesc, n).offset == out[n], n
    assert L.SourceMixDesc.rank.offset % 4 == 0          # the kernel reads a rank row as 8 dwords
    # the descriptors that existed stay what they were
    assert C.sizeof(L.ClassMixU8Desc) == 40 + 20 + 32 + 32 + 1024 + 4 and C.sizeof(L.ClassMixDesc) == 40 + 16 + 32 + 32 + 1024


def test_signatures():
    p = C.c_void_p
    assert L.SIGNATURES["simt_source_mix"] == (C.c_int, [C.POINTER(L.SourceMixDesc), p])
    assert L.SIGNATURES["simt_source_mix_items"] == (C.c_int, [C.POINTER(L.SourceMixDesc), p, p])
    assert L.SIGNATURES["simt_head_loss_weighted_n"] == (C.c_int, [C.POINTER(L.HeadDesc), p, C.c_int, p, p]) == L.SIGNATURES["simt_head_grad_weighted_n"]
    assert L.SIGNATURES["simt_head_loss_weighted"] == (C.c_int, [C.POINTER(L.HeadDesc), p, p, p])          # what it was


@pytest.mark.parametrize("symbol", NEW)
def test_a_library_without_a_symbol_names_it(monkeypatch, symbol):
    class Old:
        def __getattr__(self, name):
            if name == symbol:
                raise AttributeError(name)
            return lambda *a: L.ABI_VERSION
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L.C, "CDLL", lambda path: Old())
    monkeypatch.setattr(L, "LIB_PATH", __file__)
    with pytest.raises(L.SimtHipError, match=symbol + r"\b.*rebuild"):
        L.load()


# ---- the keyword ------------------------------------------------------------------------------------------------------------------------------------
def test_check_source_starts_with_the_keyword():
    assert ol.check_source(None, None) is False and ol.check_source(False, None) is False and ol.check_source(False, 0.9) is False
    assert ol.check_source(True, 0.0) is True and ol.check_source(np.bool_(True), 0.9) is True
    for v in (1, 0, "yes", 0.5, "True", [True]):
        with pytest.raises(ValueError, match=r"^online_source "):
            ol.check_source(v, 0.9)
    with pytest.raises(ValueError, match=r"^online_source needs online_labels"):
        ol.check_source(True, None)
    # the pinned functions are what they were
    assert ol.check_settings(0.5, None, None) == (0.5, None) and ol.check_mix(None, 0, None, 1, 300) == (None, 0)
    assert ol.check_weighted(None, None, None, 300) is None


def test_step_arguments_are_refused_without_the_keyword_and_required_with_it():
    class T(ol.OnlineLabelMixin):
        B, H, W = 2, 4, 6
    t = T()
    assert t._sources(None, None, 2) == ([None, None], [None, None])          # a trainer from before the keyword: no attribute at all
    t.online_source = False
    x, lab = torch.zeros(2, 3, 4, 6), torch.zeros(2, 4, 6, dtype=torch.int64)
    for a, b in ((x, lab), (x, None), (None, lab)):
        with pytest.raises(ValueError, match="online_source"):
            t._sources(a, b, 1)
    t.online_source = True
    for a, b in ((None, None), (x, None), (None, lab)):
        with pytest.raises(ValueError, match="online_source"):
            t._sources(a, b, 1)
    assert t._sources(x, lab, 1) == ([x], [lab]) and t._sources([x, x], (lab, lab), 2) == ([x, x], [lab, lab])
    with pytest.raises(ValueError, match=r"needs 2 source_image"):
        t._sources(x, lab, 2)
    with pytest.raises(ValueError, match="source_image of shape"):
        t._sources(torch.zeros(2, 3, 4, 5), lab, 1)
    with pytest.raises(ValueError, match="source_label of shape"):
        t._sources(x, torch.zeros(2, 4, 5, dtype=torch.int64), 1)


# ---- GTA5DataSet --------------------------------------------------------------------------------------------------------------------------------------
def _gta5_tree(root):
    """Two frames under images/ and labels/: label 0 holds every mapped id, an unmapped id (1) and 255; label 1 is a palette PNG."""
    from PIL import Image
    from simt_amd.dataset.gta5_dataset import ID_TO_TRAINID
    os.makedirs(root / "images")
    os.makedirs(root / "labels")
    ids = sorted(ID_TO_TRAINID) + [1, 255, 0, 34]
    lab0 = np.array(ids + [255] * (24 - len(ids)), dtype=np.uint8).reshape(4, 6)
    lab1 = np.array([[7, 8, 33, 2, 255, 26]] * 4, dtype=np.uint8)
    g = np.random.default_rng(0)
    rgb = [g.integers(0, 256, (4, 6, 3), dtype=np.uint8) for _ in range(2)]
    for n, (im, lab) in enumerate(zip(rgb, (lab0, lab1))):
        Image.fromarray(im).save(root / "images" / f"{n:05d}.png")
        out = Image.fromarray(lab, mode="L" if n == 0 else "P")
        if n == 1:
            out.putpalette([i % 256 for i in range(768)])
        out.save(root / "labels" / f"{n:05d}.png")
    open(root / "train.txt", "w").write("00000.png\n00001.png\n")
    return rgb, (lab0, lab1)


def test_gta5_dataset_decode_layout_and_repetition(tmp_path):
    from simt_amd.dataset.gta5_dataset import ID_TO_TRAINID, GTA5DataSet, trainid_table
    want = {7: 0, 8: 1, 11: 2, 12: 3, 13: 4, 17: 5, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10, 24: 11, 25: 12, 26: 13, 27: 14, 28: 15, 31: 16, 32: 17, 33: 18}
    assert ID_TO_TRAINID == want
    table = trainid_table()
    assert table.dtype == np.uint8 and table.shape == (256,)
    assert all(table[i] == want.get(i, 255) for i in range(256))
    rgb, labs = _gta5_tree(tmp_path)
    ds = GTA5DataSet(str(tmp_path), str(tmp_path / "train.txt"), crop_size=(6, 4), mean=(1.0, 2.0, 3.0), mirror=False)
    assert len(ds) == 2 and ds.scale_crop is None and ds.is_mirror is False and ds.crop_size == (6, 4) and ds.mean == (1.0, 2.0, 3.0)
    assert ds.files[0] == {"img": os.path.join(str(tmp_path), "images/00000.png"), "label": os.path.join(str(tmp_path), "labels/00000.png"),
                           "name": "00000.png"}
    for n in range(2):
        im, lab, name = ds.decode(n)
        assert name == f"{n:05d}.png" and im.dtype == np.uint8 and np.array_equal(im, rgb[n])
        assert lab.dtype == np.uint8 and lab.shape == (4, 6)
        assert np.array_equal(lab, np.vectorize(lambda v: want.get(int(v), 255))(labs[n]).astype(np.uint8))
    lab0 = ds.decode(0)[1].reshape(-1)
    assert lab0[:19].tolist() == list(range(19)) and set(lab0[19:].tolist()) == {255}
    assert ds.cache_key(0) == (ds.files[0]["img"], ds.files[0]["label"])
    # the reference's constructor arguments, in its order and with its defaults
    import inspect
    sig = inspect.signature(GTA5DataSet.__init__)
    assert list(sig.parameters)[:9] == ["self", "root", "list_path", "max_iters", "crop_size", "mean", "scale", "mirror", "ignore_label"]
    assert [sig.parameters[k].default for k in ("max_iters", "crop_size", "mean", "scale", "mirror", "ignore_label", "scale_crop")] == \
        [None, (321, 321), (128, 128, 128), True, True, 255, None]
    # max_iters repeats the list: ceil(max_iters / n) times
    rep = GTA5DataSet(str(tmp_path), str(tmp_path / "train.txt"), max_iters=5)
    assert len(rep) == 6 and [f["name"] for f in rep.files] == ["00000.png", "00001.png"] * 3
    assert GTA5DataSet(str(tmp_path), str(tmp_path / "train.txt"), scale_crop=["0.5", "1.0"]).scale_crop == ("0.5", "1.0")
    other = GTA5DataSet(str(tmp_path), str(tmp_path / "train.txt"), ignore_label=250)
    assert other.decode(0)[1].reshape(-1)[19:].tolist() == [250] * 5
    # a label image that is no 8-bit single-channel image is refused with its path
    from PIL import Image
    Image.fromarray(rgb[0]).save(tmp_path / "labels" / "00001.png")
    with pytest.raises(ValueError, match="00001.png: expected an 8-bit single-channel label image"):
        ds.decode(1)


# ---- the flag ---------------------------------------------------------------------------------------------------------------------------------------
def test_flag_parses_and_defaults():
    from simt_amd.tools.trainV1_warmup import balanced_kwargs, get_arguments, source_text, step_args
    a = get_arguments([])
    assert a.online_source is False and "online_source" not in balanced_kwargs(a) and source_text(a, {}) == ""
    a = get_arguments(["--online-labels", "--online-source"])
    assert a.online_source is True
    assert balanced_kwargs(a) == {"online_labels_balanced": None, "online_labels_momentum": None, "online_source": True}
    assert source_text(a, {"source_seg2": 1.23456}) == " src = 1.235"
    for model in ("DeepLab", "DeepLabv3", "DeepLabVGG"):
        a = get_arguments(["--model", model, "--online-labels", "0.9", "--online-source", "--online-mix", "0.25", "--batch-size", "32",
                           "--online-labels-weighted", "item", "--synthetic", "--ema", "--online-labels-every", "2", "--iter-size", "2",
                           "--data-dir", "/d", "--data-list", "/d/l.txt", "--scale-crop", "--random-mirror"])
        assert balanced_kwargs(a) == {"online_labels_balanced": None, "online_labels_momentum": None, "online_mix": 0.25,
                                      "online_mix_seed": 1234, "online_labels_weighted": "item", "online_source": True}
    # step_args: the source pair rides as keywords, beside the weak view when there is one
    one = get_arguments(["--online-labels", "--online-source"])
    assert step_args(one, [("x", None, None)], [("sx", "sl")]) == (("x", None), {"source_image": "sx", "source_label": "sl"})
    assert step_args(one, [("x", None, "w")], [("sx", "sl")]) == (("x", None), {"source_image": "sx", "source_label": "sl", "teacher_image": "w"})
    two = get_arguments(["--online-labels", "--online-source", "--iter-size", "2"])
    assert step_args(two, [("x", None, None), ("y", None, None)], [("sx", "sl"), ("sy", "sm")]) == \
        ((["x", "y"], None), {"source_image": ["sx", "sy"], "source_label": ["sl", "sm"]})
    # without the flag the arguments are what they were
    off = get_arguments(["--online-labels"])
    assert step_args(off, [("x", None, None)]) == (("x", None), {}) and step_args(off, [("x", None, "w")]) == (("x", None), {"teacher_image": "w"})
    assert step_args(get_arguments([]), [("x", "l")]) == (("x", "l"), {})


@pytest.mark.parametrize("argv,named", [
    (["--online-source"], "--online-source needs --online-labels"),
    (["--online-source", "--ema", "--batch-size", "2"], "--online-source needs --online-labels"),
    (["--online-labels", "--online-source", "yes"], "unrecognized arguments"),
    (["--online-labels", "--online-source", "--online-mix"], "--online-mix with --batch-size 1"),
])
def test_flag_refusals_exit_2_and_name_the_flag(capsys, argv, named):
    from simt_amd.tools.trainV1_warmup import get_arguments
    with pytest.raises(SystemExit) as e:
        get_arguments(argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and named in err, (argv, err)


def test_the_source_loader_refuses_a_missing_directory_or_list(tmp_path):
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    a = tool.get_arguments(["--online-labels", "--online-source", "--data-dir", str(tmp_path / "none")])
    with pytest.raises(SystemExit, match=r"--online-source: --data-dir .* is not a directory"):
        shared.source_batches(a, 1, 8, 8, CD.numpy(), 0, 1, "cpu")
    a = tool.get_arguments(["--online-labels", "--online-source", "--data-dir", str(tmp_path), "--data-list", str(tmp_path / "none.txt")])
    with pytest.raises(SystemExit, match=r"--online-source: --data-list .* is not a file"):
        shared.source_batches(a, 1, 8, 8, CD.numpy(), 0, 1, "cpu")
    assert shared.SOURCE_SEED_OFFSET == 0x5372


def test_the_simt_tool_gets_no_such_flag(capsys):
    from simt_amd.tools.trainV2_simt import get_arguments
    with pytest.raises(SystemExit) as e:
        get_arguments(["--online-source"])
    assert e.value.code == 2 and "unrecognized arguments" in capsys.readouterr().err


def test_start_up_lines_on_and_off(capsys):
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    shared.online_label_line(tool.get_arguments(["--online-labels"]))
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and out.endswith("the same batch as the student\n") and "online source" not in out          # the line it was
    shared.online_label_line(tool.get_arguments(["--online-labels", "0.9", "--online-source", "--synthetic"]))
    out = capsys.readouterr().out
    assert out.count("\n") == 2 and out.splitlines()[1].startswith("online source: one optimiser step = (1) supervised cross-entropy on a labelled source batch")
    assert "pasted" not in out and "--random-mirror and --scale-crop only" in out
    shared.online_label_line(tool.get_arguments(["--online-labels", "0.9", "--online-source", "--online-mix", "0.5", "--batch-size", "2",
                                                  "--online-labels-weighted"]))
    out = capsys.readouterr().out
    assert "a target item receives, image and ground truth, half of the classes of its source item" in out and "its neighbour" not in out
    assert "weighted by q" in out and "ground truth and weight 1 where pasted" in out
    assert "--online-source (needs --online-labels; DESIGN 7.20)" in tool.__doc__ and " src = <loss_seg2 of the source pass>" in tool.__doc__


# ---- run identity and the train-state file ------------------------------------------------------------------------------------------------------------
def test_run_identity_carries_the_flag_only_when_it_is_on(tmp_path):
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    cd = CD.numpy()
    off = shared.run_identity(tool.get_arguments([]), cd)
    one = shared.run_identity(tool.get_arguments(["--online-labels"]), cd)
    on = shared.run_identity(tool.get_arguments(["--online-labels", "--online-source", "--data-list", str(tmp_path / "none.txt")]), cd)
    assert "online_source" not in off and "online_source" not in one and on["online_source"] is True
    assert {k: v for k, v in on.items() if k != "online_source"} == one
    assert shared.RUN_DEFAULTS["online_source"] is False
    open(tmp_path / "l.txt", "w").write("a.png\n")
    listed = shared.run_identity(tool.get_arguments(["--online-labels", "--online-source", "--data-list", str(tmp_path / "l.txt")]), cd)
    import hashlib
    assert listed["source_list_sha256"] == hashlib.sha256(b"a.png\n").hexdigest()


def test_train_state_file_refuses_the_flag_added_or_dropped(tmp_path, no_device_sync):
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    cd = CD.numpy()
    base = ["--ema", "0.9", "--train-state", str(tmp_path / "s.state"), "--online-labels", "0.9", "--batch-size", "2", "--synthetic"]

    class Keeper:
        def state(self):
            return {}

        def load_state(self, s):
            pass
    on = ["--online-source"]
    for first, second in ((on, []), ([], on)):
        if os.path.exists(tmp_path / "s.state"):
            os.remove(tmp_path / "s.state")
        shared.TrainStateFile(tool.get_arguments(base + first), 0, 1, cd).write(_advanced(_Fake(ema_decay=0.9)), Keeper())
        assert shared.TrainStateFile(tool.get_arguments(base + first), 0, 1, cd).resume(_Fake(ema_decay=0.9, seed=1), Keeper()) == 3
        with pytest.raises(SystemExit, match="online_source"):
            shared.TrainStateFile(tool.get_arguments(base + second), 0, 1, cd).resume(_Fake(ema_decay=0.9, seed=1), Keeper())


# ---- train state on fake trainers -----------------------------------------------------------------------------------------------------------------
def _FakeSource(on=None, seed=0, **kw):
    tr = _FakeWeighted(seed=seed, **kw)
    if on is not None:
        tr.online_source = on
    if on:
        tr.source_hout = torch.zeros(2)
    return tr


def test_hyper_and_accumulators_carry_the_keyword_only_when_on(no_device_sync):
    legacy = _advanced(_FakeWeighted()).training_state()          # a fake from before the keyword: no attribute at all
    off = _advanced(_FakeSource(False)).training_state()
    assert legacy["hyper"] == off["hyper"] and legacy.keys() == off.keys()
    assert set(legacy["accumulators"]) == set(off["accumulators"]) == {"hout", "bad_labels", "label_counts", "counts_reported"}
    assert not set(off["hyper"]) & set(tsf.SOURCE_FIELDS) and tsf.SOURCE_FIELDS == ("online_source",)
    # the field lists that existed are what they were
    assert tsf.MIX_FIELDS == ("online_mix", "online_mix_seed") and tsf.VALUE_FIELDS == ("online_labels", "online_labels_every")
    assert tsf.BALANCE_FIELDS == ("online_labels_balanced", "online_labels_momentum") and tsf.WEIGHTED_FIELDS == ("online_labels_weighted",)
    on_tr = _advanced(_FakeSource(True))
    on_tr.source_hout.copy_(torch.tensor([0.5, 1.25]))
    on = on_tr.training_state()
    assert on["hyper"]["online_source"] is True
    assert {k: v for k, v in on["hyper"].items() if k != "online_source"} == off["hyper"]
    assert set(on["accumulators"]) == set(off["accumulators"]) | {"source_hout"} and set(on) == set(off)
    # added or dropped: the field is named with both values
    _refused(_FakeSource(False, seed=1), on, "online_source (state: True, this trainer: None)")
    _refused(_FakeWeighted(seed=1), on, "online_source (state: True, this trainer: None)")          # a trainer from before the keyword
    _refused(_FakeSource(True, seed=1), off, "online_source (state: None, this trainer: True)")
    _refused(_FakeSource(True, seed=1), legacy, "online_source (state: None, this trainer: True)")
    tr = _FakeSource(True, seed=1)
    tr.load_training_state(on)
    assert tr.it_done == 3 and tr.source_hout.tolist() == [0.5, 1.25]
    for ts, t in ((legacy, _FakeSource(False, seed=1)), (off, _FakeWeighted(seed=1))):
        t.load_training_state(ts)
        assert t.it_done == 3
    both = _advanced(_FakeSource(True, mode="item", mix=0.5)).training_state()
    assert both["hyper"]["online_mix"] == 0.5 and both["hyper"]["online_labels_weighted"] == "item" and both["hyper"]["online_source"] is True
    assert tsf.value_mismatches({"online_source": True}, {}) == []          # the default fields are the two they were
    assert tsf.value_mismatches({"online_source": True}, {}, fields=tsf.SOURCE_FIELDS) == ["online_source"]


def test_num_batches_tracked_counts_two_forwards_per_micro_batch():
    class Hp:
        iter_size = 3

    class T(tsf.TrainStateMixin):
        hp, it_done = Hp(), 5
    t = T()
    assert t._nbt_steps("bn1.num_batches_tracked") == 15
    t.online_source = False
    assert t._nbt_steps("bn1.num_batches_tracked") == 15
    t.online_source = True
    assert t._nbt_steps("bn1.num_batches_tracked") == 30
    t.model = "vgg"
    assert t._nbt_steps("bn1.num_batches_tracked") == 0
