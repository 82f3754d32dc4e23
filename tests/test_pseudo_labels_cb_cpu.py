"""Host side of the class-balanced pseudo-label export (make_pseudo_labels --class-balanced): the bindings of simt_pseudo_conf_u8 /
simt_pseudo_conf2_u8 against their header declarations, class_thresholds against a sort-based restatement of the BDL rule, the
argument checks that run before any GPU work and the thresholds file."""
import json
import os
import re

import numpy as np
import pytest

from simt_amd import _lib as L
from simt_amd.tools import make_pseudo_labels as mpl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "simt_hip.h")).read()


def _params(name):
    m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", HDR)
    assert m, f"{name} is not declared in include/simt_hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _kinds(params):
    kinds = []
    for p in params:
        if "*" in p or p.startswith("simt_stream_t"):
            kinds.append("ptr")
        elif p.split()[0] == "float":
            kinds.append("float")
        else:
            assert p.split()[0] == "int", p
            kinds.append("int")
    return kinds


@pytest.mark.parametrize("name,label,ngeo", [("simt_pseudo_conf_u8", "simt_pseudo_label_u8", 4),
                                             ("simt_pseudo_conf2_u8", "simt_pseudo_label2_u8", 6)])
def test_conf_bindings_match_header(name, label, ngeo):
    assert L.ABI_VERSION == 2 and int(re.search(r"#define\s+SIMT_ABI_VERSION\s+(\d+)", HDR).group(1)) == 2   # symbols added, no layout change
    params = _params(name)
    res, args = L.SIGNATURES[name]
    assert res is L.C.c_int
    got = ["ptr" if a is L.C.c_void_p else "int" if a is L.C.c_int else "float" if a is L.C.c_float else repr(a) for a in args]
    assert got == _kinds(params)
    names = [p.split()[-1].lstrip("*") for p in params]
    old = [p.split()[-1].lstrip("*") for p in _params(label)]
    # the first scale's geometry of the label kernel, then B H W C and the class-balanced tail
    assert names[:ngeo] == old[:ngeo]
    assert names[ngeo:] == ["B", "H", "W", "C", "thr", "out", "counts", "hist", "stream"]
    assert len(names) == ngeo + 9


def test_conf_bins_constant():
    assert int(re.search(r"#define\s+SIMT_CONF_BINS\s+(\d+)", HDR).group(1)) == L.CONF_BINS == mpl.CONF_BINS == 256


def test_a_library_without_the_symbols_names_them(monkeypatch):
    """A libsimt_hip.so built before the symbols were added has the same ABI version: loading must name the symbol and say to rebuild."""
    class Old:
        def __getattr__(self, name):
            if name.startswith("simt_pseudo_conf"):
                raise AttributeError(name)
            fn = lambda *a: L.ABI_VERSION     # noqa: E731
            return fn
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L.C, "CDLL", lambda path: Old())
    monkeypatch.setattr(L, "LIB_PATH", __file__)
    with pytest.raises(L.SimtHipError, match=r"simt_pseudo_conf2?_u8.*rebuild"):
        L.load()


# ---- class_thresholds ------------------------------------------------------------------------------------------------------------------
def _bins(x):
    return np.minimum(255, np.floor(x * np.float32(256)).astype(np.int64))


def _hist(x):
    return np.bincount(_bins(x), minlength=256)


def _draw(rng):
    """Confidences of one class, float32 in [0, 1]: a random shape, sometimes with a mass at exactly 1.0 or on bin edges."""
    n = int(rng.integers(1, 4000))
    kind = rng.integers(0, 4)
    if kind == 0:
        x = rng.random(n, dtype=np.float32)
    elif kind == 1:
        x = (1 - rng.random(n, dtype=np.float32) ** 4).astype(np.float32)        # crowded near 1
    elif kind == 2:
        x = (rng.integers(0, 257, n) / 256).astype(np.float32)                  # exactly on bin edges, 1.0 included
    else:
        x = (rng.random(n, dtype=np.float32) * np.float32(0.3) + np.float32(0.05)).astype(np.float32)
    if rng.random() < 0.3:
        x[rng.random(n) < 0.6] = 1.0
    return x


def test_class_thresholds_against_sorted_rule():
    rng = np.random.default_rng(5)
    draws = [_draw(rng) for _ in range(199)]
    hot = rng.random(3000, dtype=np.float32)
    hot[:1800] = 1.0                                                            # 60 % of the mass at exactly 1.0
    draws.append(hot)
    for i, x in enumerate(draws):
        portion = [0.5, 0.2, 0.8, 1.0, 0.05][i % 5] if i % 7 else float(rng.uniform(0.01, 1.0))
        n = len(x)
        h = _hist(x)
        k = min(int(np.round(n * (1 - portion))), n - 1)                        # BDL: x_sorted[round(n * 0.5)]
        xs = np.sort(x)
        t = mpl.class_thresholds(h[None], portion, cap=2.0)[0]                  # uncapped
        assert t.dtype == np.float32
        b = int(round(float(t) * 256))
        assert np.float32(b / 256) == t, "the threshold is a bin's lower edge"
        assert t <= xs[k] and (xs[k] < t + np.float32(1 / 256) or xs[k] == 1)   # the top bin also holds 1.0 itself (the clamp)
        kept = int((x >= t).sum())
        assert kept == int(h[b:].sum())
        assert n - k <= kept < n - k + h[b]
        below = np.nextafter(t, np.float32(-np.inf))
        assert np.array_equal(x >= t, x > below)                                # the strict rule of the confidence mode
        if i == len(draws) - 1:
            assert t == np.float32(255 / 256) and kept == 1800 + int((hot[1800:] >= t).sum())


def test_class_thresholds_edge_cases():
    rng = np.random.default_rng(6)
    x = rng.random(1000, dtype=np.float32)
    h = np.stack([_hist(x), np.zeros(256, np.int64), _hist(np.full(7, 0.97, np.float32))])
    t = mpl.class_thresholds(h, 0.5, cap=0.9)
    assert t[1] == 0                                                            # an empty class
    assert t[2] == np.float32(0.9) and t.dtype == np.float32                    # the cap, exactly float32(cap)
    # portion = 1 keeps everything: k = 0, so the threshold is the lower edge of the class's lowest occupied bin -- 0 for a class with
    # a pixel below 1/256 (and for an empty one), and never above the class's minimum
    assert x.min() < 1 / 256
    all_ = mpl.class_thresholds(h, 1.0, cap=1.0)
    assert all_[0] == 0 and all_[1] == 0 and all_[2] == np.float32(248 / 256) <= np.float32(0.97)
    # k clamped to n - 1: round(n * (1 - P)) reaches n for a small share
    one = _hist(np.array([0.3], np.float32))[None]
    assert int(np.round(1 * (1 - 0.01))) == 1
    assert mpl.class_thresholds(one, 0.01, cap=1.0)[0] == np.float32(76 / 256)
    # half-to-even, as np.round: n = 5, P = 0.5 -> k = round(2.5) = 2
    five = _hist(np.array([0.1, 0.2, 0.3, 0.4, 0.5], np.float32))[None]
    assert mpl.class_thresholds(five, 0.5, cap=1.0)[0] == np.float32(76 / 256)
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            mpl.class_thresholds(h, bad)


# ---- command line ----------------------------------------------------------------------------------------------------------------------
def test_arguments():
    a = mpl.get_arguments(["--restore-from", "m.pth", "--class-balanced", "0.5"])
    assert a.class_balanced == 0.5 and a.threshold_cap == 0.9 and a.threshold is None and a.thresholds_from is None
    a = mpl.get_arguments(["--restore-from", "m.pth", "--class-balanced", "1", "--threshold-cap", "1.0"])
    assert a.class_balanced == 1.0 and a.threshold_cap == 1.0
    with pytest.raises(SystemExit):
        mpl.get_arguments(["--restore-from", "m.pth", "--class-balanced", "0.5", "--threshold", "0.8"])
    with pytest.raises(SystemExit):
        mpl.get_arguments(["--restore-from", "m.pth", "--thresholds-from", "t.json", "--threshold", "0.8"])
    for bad in ("0", "-0.5", "1.01", "nan"):
        with pytest.raises(SystemExit):
            mpl.get_arguments(["--restore-from", "m.pth", "--class-balanced", bad])
    with pytest.raises(SystemExit):
        mpl.get_arguments(["--restore-from", "m.pth", "--class-balanced", "0.5", "--threshold-cap", "0"])
    with pytest.raises(SystemExit):
        mpl.get_arguments(["--restore-from", "m.pth", "--class-balanced", "0.5", "--num-classes", "65"])


def _record(C=19, seed=0):
    rng = np.random.default_rng(seed)
    hist = rng.integers(0, 1000, (C, 256))
    hist[3] = 0
    thr = mpl.class_thresholds(hist, 0.5, 0.9)
    counts = np.array([int(hist[c][int(round(float(thr[c]) * 256)):].sum()) for c in range(C)] + [0])
    return thr, hist, mpl.thresholds_record(thr, counts, hist, portion=0.5, cap=0.9, data_list="train.txt")


def test_thresholds_file_round_trip(tmp_path):
    thr, hist, rec = _record()
    path = mpl.thresholds_path(str(tmp_path / "lists" / "p.lst"), "pseudo_x")
    assert path == str(tmp_path / "lists" / "pseudo_x_thresholds.json")
    os.makedirs(os.path.dirname(path))
    mpl.save_json_atomic(rec, path)
    assert os.listdir(os.path.dirname(path)) == ["pseudo_x_thresholds.json"]    # no temporary file left
    got, back = mpl.load_thresholds(path, 19)
    assert got.dtype == np.float32 and np.array_equal(got, thr)                 # float32 -> JSON -> float32 is exact
    assert back == json.loads(json.dumps(rec))
    assert back["num_classes"] == 19 and back["bins"] == 256 and back["portion"] == 0.5 and back["cap"] == 0.9
    assert back["data_list"] == "train.txt"
    for c, e in enumerate(back["classes"]):
        assert e["class"] == c and e["pixels"] == int(hist[c].sum()) and e["hist"] == [int(v) for v in hist[c]]
        assert e["kept_share"] == (e["kept"] / e["pixels"] if e["pixels"] else None)
    assert back["classes"][3]["pixels"] == 0 and back["classes"][3]["threshold"] == 0


@pytest.mark.parametrize("field,value", [("num_classes", 16), ("bins", 128)])
def test_mismatching_thresholds_file_is_refused(tmp_path, field, value):
    _, _, rec = _record()
    rec[field] = value
    path = str(tmp_path / "t.json")
    mpl.save_json_atomic(rec, path)
    with pytest.raises(ValueError, match=field):
        mpl.load_thresholds(path, 19)
    # the command line refuses it before the checkpoint is read or the GPU is touched
    with pytest.raises(SystemExit, match=field):
        mpl.main(["--restore-from", str(tmp_path / "missing.pth"), "--data-dir", "unused", "--thresholds-from", path])
    with pytest.raises(SystemExit, match="thresholds-from"):
        mpl.main(["--restore-from", str(tmp_path / "missing.pth"), "--data-dir", "unused", "--thresholds-from", str(tmp_path / "none.json")])
