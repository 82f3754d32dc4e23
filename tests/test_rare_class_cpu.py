"""Rare-class sampling without a GPU: the sampler (simt_amd/data/rare_class.py) against its restatement
(tests/_rare_crop_ref.py), the statistics tool on PNG files, the restatement of the device contract on hand-made frames, the header,
descriptors and signatures, the flags of trainV1_warmup with their refusals, the run identity, and the K-candidate skip function."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

import _rare_crop_ref as rref
import _scale_crop_ref as scref
from oracle import simt_oracle as so
from simt_amd import _lib as L
from simt_amd.data import rare_class as rc
from simt_amd.data import scale_crop as sc
from test_ema_cpu import _advanced, _Fake, no_device_sync  # noqa: F401  (the fixture is used by name)
from test_online_labels_cb_cpu import _layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "simt_hip.h")).read()
CD = so.load_class_dist()
NEW = ["simt_rare_crop_counts", "simt_rare_crop_pick", "simt_scale_crop_win"]


# ---- the sampler --------------------------------------------------------------------------------------------------------------------------------
def _counts_spanning():
    """12 frames, 7 classes: frequencies 0.4, 0.35, 0.2, ~0.05, 1e-3, 1e-4, 1e-5 of 10^7 pixels a frame; class 6 never reaches 3000 pixels in
    one frame (100 a frame), class 5 does in two frames only."""
    per = np.array([4_000_000, 3_500_000, 2_000_000, 488_900, 10_000, 0, 100], dtype=np.int64)
    counts = np.tile(per, (12, 1))
    counts[3, 5] = counts[7, 5] = 6_000
    counts[:, 4] = [0, 0, 0, 40_000, 0, 40_000, 0, 0, 40_000, 0, 0, 0]
    return counts


@pytest.mark.parametrize("T", [0.01, 1.0])
def test_class_probs_equal_the_restatement(T):
    counts = _counts_spanning()
    f = counts.sum(0) / counts.sum()
    assert f.max() == pytest.approx(0.4, rel=1e-3) and 0.9e-5 < f[6] < 1.1e-5 and 0.9e-4 < f[5] < 1.1e-4
    P = rc.class_probs(counts, T, 3000)
    R = rref.class_probs(counts, T, 3000)
    assert P.dtype == np.float64 and np.allclose(P, R, rtol=1e-12, atol=0.0) and abs(P.sum() - 1.0) < 1e-12
    assert P[6] == 0.0 and (P[:6] > 0).all()                     # class 6: no frame holds 3000 pixels of it
    assert [l.tolist() for l in rc.items_with_class(counts, 3000)] == rref.items_with_class(counts, 3000)
    assert rc.items_with_class(counts, 3000)[5].tolist() == [3, 7] and rc.items_with_class(counts, 3000)[6].tolist() == []
    if T == 0.01:                                               # the rarest qualifying classes carry the mass
        assert P[4] + P[5] > 0.99 and P[0] < 1e-15


def test_class_probs_refusals():
    counts = _counts_spanning()
    for T in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            rc.class_probs(counts, T, 3000)
    with pytest.raises(ValueError, match="no class has a frame"):
        rc.class_probs(counts, 0.01, 10 ** 9)


def test_draws_are_reproducible_and_skippable_and_equal_the_restatement():
    counts = _counts_spanning()
    r = rc.RareClass(counts, T=1.0, min_pixels=3000)
    a = [rc.draw_batch(rc.generator(5, 1), 4, r.cdf, r.lists) for _ in range(2)]
    assert a[0] == a[1]
    g = rc.generator(5, 1)
    seq = [rc.draw_batch(g, 4, r.cdf, r.lists) for _ in range(6)]
    for n in (0, 1, 5):
        assert rc.draw_batch(rc.skip_draws(rc.generator(5, 1), 4, n), 4, r.cdf, r.lists) == seq[n]
    gr = rref.generator(5, 1)
    assert seq == [tuple(rref.draw_batch(gr, 4, rref.class_probs(counts, 1.0, 3000), rref.items_with_class(counts, 3000))) for _ in range(6)]
    assert rc.draw_batch(rc.generator(5, 0), 4, r.cdf, r.lists) != seq[0]                 # another rank, another stream
    # exactly two draws per batch: random(B), random(B)
    g, h = rc.generator(9, 0), rc.generator(9, 0)
    rc.draw_batch(g, 3, r.cdf, r.lists)
    h.random(3), h.random(3)
    assert g.random() == h.random()


def test_draws_follow_the_probabilities_and_frames_are_uniform():
    """20 000 draws, seed fixed: every class's share within 4 standard deviations of P, every frame's share within its class likewise."""
    counts = _counts_spanning()
    r = rc.RareClass(counts, T=0.25, min_pixels=3000)
    assert (r.probs[:6] > 0.01).all() and r.probs[6] == 0
    g = rc.generator(1234, 0)
    cls, idx = [], []
    for _ in range(2500):
        c, i = rc.draw_batch(g, 8, r.cdf, r.lists)
        cls += c
        idx += i
    cls, idx, n = np.array(cls), np.array(idx), 20000
    assert len(cls) == n and (cls != 6).all()
    for c in range(7):
        p = r.probs[c]
        assert abs((cls == c).sum() - n * p) <= 4 * np.sqrt(n * p * (1 - p)), c
        m, items = int((cls == c).sum()), r.lists[c]
        if m:
            assert set(idx[cls == c].tolist()) <= set(items.tolist())
            q = 1.0 / len(items)
            for i in items:
                assert abs((idx[cls == c] == i).sum() - m * q) <= 4 * np.sqrt(m * q * (1 - q)) + 1e-9, (c, i)


def test_parse_validates_and_computes_min_count_exactly():
    assert rc.parse("0.01", "3000", "0.5", "10") == (0.01, 3000, "0.5", 10, 1500)
    assert rc.parse(0.5, 3000, "0.7", 16)[4] == 2100 and rc.parse(0.5, 10, "0.29", 1)[4] == 2          # 10 * 0.29 = 2.9, not 2.9000000000000004
    assert rc.parse(1, 0, "1", 1)[4] == 0 and rc.parse(1, 7, "0", 1)[4] == 0 and rc.parse(1, 1000, "0.7", 1)[4] == rref.min_count(1000, "0.7")
    for bad, named in ((("0", 1, "0.5", 1), "temperature"), (("x", 1, "0.5", 1), "temperature"), ((1, -1, "0.5", 1), "--rcs-min-pixels"),
                       ((1, "1.5", "0.5", 1), "--rcs-min-pixels"), ((1, 1, "1.01", 1), "--rcs-min-crop-ratio"), ((1, 1, "-0.1", 1), "--rcs-min-crop-ratio"),
                       ((1, 1, "1/2", 1), "--rcs-min-crop-ratio"), ((1, 1, "0.5", 0), "--rcs-crops"), ((1, 1, "0.5", 17), "--rcs-crops"),
                       ((1, 1, "0.5", "k"), "--rcs-crops")):
        with pytest.raises(ValueError, match=named):
            rc.parse(*bad)


# ---- the statistics tool ----------------------------------------------------------------------------------------------------------------------------
def _gta5_files(root, n=8, hw=(12, 20)):
    """n frames under images/ and labels/ with GTA5 ids: mapped ids, an unmapped id (1), 255; frame 2 is all ignore."""
    from PIL import Image
    from simt_amd.dataset.gta5_dataset import ID_TO_TRAINID
    os.makedirs(root / "images")
    os.makedirs(root / "labels")
    g = np.random.default_rng(3)
    ids = np.array(sorted(ID_TO_TRAINID) + [1, 255], dtype=np.uint8)
    labs = []
    for i in range(n):
        lab = ids[g.integers(0, len(ids), hw)]
        if i == 2:
            lab[:] = 255
        Image.fromarray(g.integers(0, 256, hw + (3,), dtype=np.uint8)).save(root / "images" / f"{i:05d}.png")
        Image.fromarray(lab).save(root / "labels" / f"{i:05d}.png")
        labs.append(lab)
    open(root / "train.txt", "w").write("".join(f"{i:05d}.png\n" for i in range(n)))
    return labs


def test_statistics_tool_counts_the_mapped_labels_and_the_loader_refuses_another_list(tmp_path, capsys):
    pytest.importorskip("PIL.Image")
    from simt_amd.dataset.gta5_dataset import ID_TO_TRAINID, GTA5DataSet
    from simt_amd.tools import compute_class_stats as tool
    labs = _gta5_files(tmp_path)
    out = tmp_path / "stats.json"
    tool.main(["--data-dir", str(tmp_path), "--data-list", str(tmp_path / "train.txt"), "--out", str(out), "--num-workers", "2"])
    assert "8 frames" in capsys.readouterr().out
    doc = json.load(open(out))
    assert doc["n_classes"] == 19 and doc["ignore_label"] == 255 and len(doc["items"]) == 8
    assert doc["list_sha256"] == hashlib.sha256(open(tmp_path / "train.txt", "rb").read()).hexdigest()
    assert [f for f in os.listdir(tmp_path) if f.endswith(".tmp")] == []
    for i, it in enumerate(doc["items"]):
        mapped = np.vectorize(lambda v: ID_TO_TRAINID.get(int(v), 255))(labs[i]).astype(np.int64).reshape(-1)
        assert it["name"] == f"{i:05d}.png" and it["counts"] == np.bincount(mapped[mapped < 19], minlength=19).tolist()
    assert sum(doc["items"][2]["counts"]) == 0 and sum(doc["items"][0]["counts"]) < 12 * 20          # all ignore; unmapped ids are not counted
    ds = GTA5DataSet(str(tmp_path), str(tmp_path / "train.txt"))
    counts = rc.load_stats(str(out), ds)
    assert counts.shape == (8, 19) and counts.dtype == np.int64 and counts.tolist() == [it["counts"] for it in doc["items"]]
    # 5 classes only: the higher train ids are not counted
    tool.main(["--data-dir", str(tmp_path), "--data-list", str(tmp_path / "train.txt"), "--out", str(tmp_path / "s5.json"), "--num-classes", "5"])
    assert [it["counts"] for it in json.load(open(tmp_path / "s5.json"))["items"]] == [it["counts"][:5] for it in doc["items"]]
    # another list: refused, the first difference named
    open(tmp_path / "other.txt", "w").write("".join(f"{i:05d}.png\n" for i in (0, 1, 3, 2, 4, 5, 6, 7)))
    with pytest.raises(ValueError, match=r"item 2 is '00002.png', the dataset's list has '00003.png'"):
        rc.load_stats(str(out), GTA5DataSet(str(tmp_path), str(tmp_path / "other.txt")))
    open(tmp_path / "short.txt", "w").write("".join(f"{i:05d}.png\n" for i in range(7)))
    with pytest.raises(ValueError, match=r"8 items, the dataset's list has 7"):
        rc.load_stats(str(out), GTA5DataSet(str(tmp_path), str(tmp_path / "short.txt")))
    assert GTA5DataSet(str(tmp_path), str(tmp_path / "train.txt")).rare_class is None
    r = rc.RareClass(counts, T=1.0, min_pixels=1)
    assert GTA5DataSet(str(tmp_path), str(tmp_path / "train.txt"), rare_class=r).rare_class is r


# ---- the restatement of the device contract, against itself on hand-made frames ------------------------------------------------------------------------
def test_restatement_on_hand_made_frames():
    pytest.importorskip("PIL.Image")
    crop = (8, 6)
    lab = np.zeros((12, 16), np.uint8)                  # choice "2.0": the scaled label IS the frame (16 x 12), origins 0..8 x 0..6
    lab[9:, 12:] = 5                                    # class 5 sits in the bottom right corner: 3 x 4 pixels
    lab[0, 0] = 255
    memo = {}
    cand = ([[0, 0, 0]], [[0, 8, 6]], [[0, 6, 6]])      # (pick, ox, oy): top left; bottom right, all 12 pixels; two of the corner's four columns
    counts, ks, win = rref.windows(memo, ["a"], [lab], crop, ("2.0",), cand, [5], 0)
    assert counts == [[0, 12, 6]] and ks == [1] and win == [[0, 8, 6, 12]]
    assert rref.windows(memo, ["a"], [lab], crop, ("2.0",), cand, [5], 11)[1] == [1]          # 12 > 11
    assert rref.windows(memo, ["a"], [lab], crop, ("2.0",), cand, [5], 12)[1:] == ([2], [[0, 6, 6, 6]])      # none passes: K - 1
    assert rref.windows(memo, ["a"], [lab], crop, ("2.0",), cand, [255], 0)[1:] == ([0], [[0, 0, 0, 0]])     # class 255: candidate 0, nothing counted
    assert rref.windows(memo, ["a"], [lab], crop, ("2.0",), cand, [7], 0)[0] == [[0, 0, 0]]                  # an absent class
    # a frame smaller than the crop ("0.5": 4 x 3 placed inside 8 x 6): the padding is not counted, whatever the class
    full = np.full((12, 16), 3, np.uint8)
    assert rref.count(memo, "b", full, crop, "0.5", -2, -1, 3) == 12 and rref.count(memo, "b", full, crop, "0.5", -4, -3, 255) == 0
    # the count is the label of _scale_crop_ref.item at that window
    rgb = np.zeros((12, 16, 3), np.uint8)
    for (ox, oy) in ((0, 0), (8, 6), (6, 6)):
        _x, lo = scref.item(scref.Resized(), "a", rgb, lab, crop, "2.0", ox, oy, True)
        assert int((lo == 5).sum()) == rref.count(memo, "a", lab, crop, "2.0", ox, oy, 5)


# ---- header, descriptors, signatures ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_symbols_and_the_descriptor_matches_ctypes():
    for name in NEW:
        assert re.search(rf"int {name}\(const simt_rare_crop_desc\* d, simt_stream_t stream\);", HDR)
        assert L.SIGNATURES[name] == (C.c_int, [C.POINTER(L.RareCropDesc), C.c_void_p])
    assert L.ABI_VERSION == 2 and int(re.search(r"#define\s+SIMT_ABI_VERSION\s+(\d+)", HDR).group(1)) == 2
    for name, v in (("MAX", L.RARE_CROP_MAX), ("CANDS", L.RARE_CROP_CANDS), ("PARTS", L.RARE_CROP_PARTS)):
        assert v == 16 == int(re.search(rf"#define SIMT_RARE_CROP_{name} (\d+)", HDR).group(1))
    assert rc.MAX_CANDS == L.RARE_CROP_CANDS and rref.PARTS == L.RARE_CROP_PARTS
    names = [n for n, _t in L.RareCropDesc._fields_]
    assert names == ["img", "lab", "cand_ox", "cand_oy", "cand_choice", "mirror", "cls", "c", "tables", "x", "lab_out", "parts", "win", "B", "Hs",
                     "Ws", "h", "w", "n_choices", "max_rows", "n_tables", "K", "min_count", "mean"]
    out = _layout("simt_rare_crop_desc", names)
    assert C.sizeof(L.RareCropDesc) == out["size"] < 4096          # it travels as kernel arguments
    for n in names:
        assert getattr(L.RareCropDesc, n).offset == out[n], n
    # everything simt_scale_crop_desc holds except ox, oy and choice
    assert {n for n, _t in L.ScaleCropDesc._fields_} - set(names) == {"ox", "oy", "choice"}
    # the scale-crop descriptor is what it was
    assert C.sizeof(L.ScaleCropDesc) == 2376 == _layout("simt_scale_crop_desc", ["img"])["size"] and L.SCALE_CROP_MAX == 64


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


# ---- the loader's generator: K candidates --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror", [False, True])
def test_candidate_draws_equal_the_restatement_and_the_skip_advances_alike(mirror):
    choices, crop = ("0.5", "1.0", "1.5"), (72, 40)
    g, r = np.random.default_rng(77), np.random.default_rng(77)
    seq = [sc.draw_batch_candidates(g, 3, 4, choices, crop, mirror) for _ in range(5)]
    assert seq == [rref.cand_draws(r, 3, 4, choices, crop, mirror) for _ in range(5)]
    assert all(len(row) == 4 for d in seq for rows in d[1:] for row in rows)
    for n in (0, 2, 4):
        s = sc.skip_scale_crop_draws(np.random.default_rng(77), 3, n, len(choices), mirror, candidates=4)
        assert sc.draw_batch_candidates(s, 3, 4, choices, crop, mirror) == seq[n]
    # the single-candidate skip is what it was: the draws of draw_batch, whether or not the keyword is spelled
    a = sc.skip_scale_crop_draws(np.random.default_rng(5), 3, 4, len(choices), mirror)
    b = sc.skip_scale_crop_draws(np.random.default_rng(5), 3, 4, len(choices), mirror, candidates=None)
    c = np.random.default_rng(5)
    for _ in range(4):
        sc.draw_batch(c, 3, choices, crop, mirror)
    assert a.random() == b.random() == c.random()


# ---- the flags ----------------------------------------------------------------------------------------------------------------------------------------
BASE = ["--online-labels", "--online-source"]


def test_flags_parse_and_default():
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    a = tool.get_arguments(BASE)
    assert a.rare_class_sampling is None and shared.rare_class_setting(a) is None
    a = tool.get_arguments(BASE + ["--rare-class-sampling", "--rcs-stats", "s.json"])
    assert a.rare_class_sampling == "0.01" and shared.rare_class_setting(a) == (0.01, 3000, "0.5", 10, 1500)
    a = tool.get_arguments(BASE + ["--rare-class-sampling", "0.5", "--rcs-stats", "s.json", "--rcs-min-pixels", "100", "--rcs-min-crop-ratio", "0.25",
                                   "--rcs-crops", "4"])
    assert shared.rare_class_setting(a) == (0.5, 100, "0.25", 4, 25)
    a = tool.get_arguments(BASE + ["--rare-class-sampling", "--synthetic"])          # accepted: synthetic batches have no list
    assert shared.rare_class_setting(a)[3] == 10
    assert "--rare-class-sampling [T] (needs --online-source and --rcs-stats FILE; DESIGN 7.21)" in tool.__doc__ and " rcs = <share" in tool.__doc__

    class S:
        def rcs_share(self):
            return 0.75
    assert tool.rcs_text(S()) == " rcs = 0.750" and tool.rcs_text(iter(())) == "" and tool.rcs_text(None) == ""


@pytest.mark.parametrize("argv,named", [
    (["--online-labels", "--rare-class-sampling", "--rcs-stats", "s"], "--rare-class-sampling needs --online-source"),
    (BASE + ["--rare-class-sampling"], "--rare-class-sampling needs --rcs-stats"),
    (BASE + ["--rcs-stats", "s"], "--rcs-stats needs --rare-class-sampling"),
    (BASE + ["--rcs-min-pixels", "10"], "--rcs-min-pixels needs --rare-class-sampling"),
    (BASE + ["--rcs-min-crop-ratio", "0.5"], "--rcs-min-crop-ratio needs --rare-class-sampling"),
    (BASE + ["--rcs-crops", "3"], "--rcs-crops needs --rare-class-sampling"),
    (BASE + ["--rare-class-sampling", "0", "--rcs-stats", "s"], "temperature must be positive"),
    (BASE + ["--rare-class-sampling", "--rcs-stats", "s", "--rcs-crops", "17"], "--rcs-crops '17'"),
    (BASE + ["--rare-class-sampling", "--rcs-stats", "s", "--rcs-min-crop-ratio", "1.5"], "--rcs-min-crop-ratio '1.5'"),
    (BASE + ["--rare-class-sampling", "--rcs-stats", "s", "--rcs-min-pixels", "-3"], "--rcs-min-pixels '-3'"),
])
def test_flag_refusals_exit_2_and_name_the_flag(capsys, argv, named):
    from simt_amd.tools.trainV1_warmup import get_arguments
    with pytest.raises(SystemExit) as e:
        get_arguments(argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and named in err, (argv, err)


def test_the_simt_tool_gets_no_such_flag(capsys):
    from simt_amd.tools.trainV2_simt import get_arguments
    with pytest.raises(SystemExit) as e:
        get_arguments(["--rare-class-sampling"])
    assert e.value.code == 2 and "unrecognized arguments" in capsys.readouterr().err


def test_run_identity_carries_the_flag_only_when_it_is_on(tmp_path):
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    cd = CD.numpy()
    open(tmp_path / "s.json", "w").write("{}\n")
    lst = ["--data-list", str(tmp_path / "none.txt")]
    off = shared.run_identity(tool.get_arguments(BASE + lst), cd)
    on = shared.run_identity(tool.get_arguments(BASE + lst + ["--rare-class-sampling", "--rcs-stats", str(tmp_path / "s.json")]), cd)
    assert "rare_class_sampling" not in off and shared.RUN_DEFAULTS["rare_class_sampling"] is False
    assert on["rare_class_sampling"] == [0.01, 3000, "0.5", 10, hashlib.sha256(b"{}\n").hexdigest()]
    assert {k: v for k, v in on.items() if k != "rare_class_sampling"} == off
    for extra, at in ((["--rare-class-sampling", "0.02"], 0), (["--rare-class-sampling", "--rcs-min-pixels", "10"], 1),
                      (["--rare-class-sampling", "--rcs-min-crop-ratio", "0.6"], 2), (["--rare-class-sampling", "--rcs-crops", "3"], 3)):
        other = shared.run_identity(tool.get_arguments(BASE + lst + extra + ["--rcs-stats", str(tmp_path / "s.json")]), cd)["rare_class_sampling"]
        assert [i for i in range(5) if other[i] != on["rare_class_sampling"][i]] == [at]
    syn = shared.run_identity(tool.get_arguments(BASE + ["--synthetic", "--rare-class-sampling"]), cd)
    assert syn["rare_class_sampling"] == [0.01, 3000, "0.5", 10, None]
    assert "rare_class_sampling" not in shared.run_identity(tool.get_arguments(BASE + ["--synthetic"]), cd)


def test_train_state_file_refuses_the_flag_added_dropped_or_changed(tmp_path, no_device_sync):
    from simt_amd.tools import trainV1_warmup as tool
    from simt_amd.tools import trainV2_simt as shared
    cd = CD.numpy()
    base = ["--ema", "0.9", "--train-state", str(tmp_path / "s.state"), "--online-labels", "0.9", "--online-source", "--batch-size", "2", "--synthetic"]

    class Keeper:
        def state(self):
            return {}

        def load_state(self, s):
            pass
    on, hot = ["--rare-class-sampling"], ["--rare-class-sampling", "0.5"]
    for first, second in ((on, []), ([], on), (on, hot)):
        if os.path.exists(tmp_path / "s.state"):
            os.remove(tmp_path / "s.state")
        shared.TrainStateFile(tool.get_arguments(base + first), 0, 1, cd).write(_advanced(_Fake(ema_decay=0.9)), Keeper())
        assert shared.TrainStateFile(tool.get_arguments(base + first), 0, 1, cd).resume(_Fake(ema_decay=0.9, seed=1), Keeper()) == 3
        with pytest.raises(SystemExit, match="rare_class_sampling"):
            shared.TrainStateFile(tool.get_arguments(base + second), 0, 1, cd).resume(_Fake(ema_decay=0.9, seed=1), Keeper())
