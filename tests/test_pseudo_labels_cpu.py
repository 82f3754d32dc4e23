"""Host side of the pseudo-label export (simt_amd.tools.make_pseudo_labels) and of trainV2_simt --class-dist: list lines and file names in
the layout of pseudo_bapa.lst, the palette of info.json, the prior's normalisation (compute_ClassDistribution.py:92), argument parsing,
and the checks that run before any GPU work."""
import json
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from simt_amd.tools import make_pseudo_labels as mpl

NAME = "aachen/aachen_000000_000019_leftImg8bit.png"


def test_list_line_and_output_paths(tmp_path):
    assert mpl.list_line("train", NAME, "pseudo_x") == \
        "train/aachen/aachen_000000_000019_leftImg8bit.png\tpseudo_x/aachen_000000_000019_leftImg8bit.png"
    png, color = mpl.output_paths(str(tmp_path), "pseudo_x", NAME)
    assert png == str(tmp_path / "pseudo_x" / "aachen_000000_000019_leftImg8bit.png")
    assert color == str(tmp_path / "pseudo_x" / "aachen_000000_000019_leftImg8bit_color.png")


def test_list_line_is_read_by_cityscapes_pseudo(tmp_path):
    from simt_amd.dataset.cityscapes_dataset import cityscapesPseudo
    lst = tmp_path / "p.lst"
    lst.write_text(mpl.list_line("train", NAME, "pseudo_x") + "\n")
    ds = cityscapesPseudo(str(tmp_path), str(lst))
    f = ds.files[0]
    assert f["img"] == str(tmp_path / "train" / NAME)
    assert f["label"] == str(tmp_path / "pseudo_x" / "aachen_000000_000019_leftImg8bit.png")


def test_palette_from_info_json(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    colours = [[128, 64, 128], [244, 35, 232], [70, 70, 70]]
    json.dump({"classes": 3, "palette": colours}, open(tmp_path / "info.json", "w"))
    pal = mpl.read_palette(str(tmp_path))
    assert len(pal) == 768 and pal[:9] == [128, 64, 128, 244, 35, 232, 70, 70, 70] and not any(pal[9:])
    lab = np.array([[0, 1], [2, 255]], dtype=np.uint8)
    img = mpl.colorize(lab, pal)
    assert img.mode == "P" and np.array_equal(np.array(img), lab)
    assert np.array_equal(np.array(img.convert("RGB"))[0, 1], [244, 35, 232])
    mpl.save_png_atomic(img, str(tmp_path / "c.png"))
    back = Image.open(tmp_path / "c.png")
    assert back.mode == "P" and np.array_equal(np.array(back), lab)
    assert [p.name for p in tmp_path.iterdir() if p.name.endswith(".tmp")] == []
    json.dump({"classes": 3}, open(tmp_path / "info.json", "w"))
    with pytest.raises(ValueError, match="palette"):
        mpl.read_palette(str(tmp_path))


def test_class_dist_matches_compute_class_distribution(tmp_path, monkeypatch):
    """The .npy the export writes equals what compute_ClassDistribution.main writes for the same counts (its GPU count is stubbed)."""
    from simt_amd.tools import compute_ClassDistribution as ccd
    rng = np.random.default_rng(5)
    counts = rng.integers(0, 10 ** 9, 20).astype(np.int64)         # 19 classes + the 255 bin
    monkeypatch.setattr(ccd, "compute_CD", lambda *a, **k: counts[:19].astype(np.float64))
    out = tmp_path / "cd.npy"
    ccd.main(["--pred-dir", str(tmp_path), "--out", str(out)])
    ref = np.load(out)
    got = mpl.class_dist(counts, 19)
    assert got.dtype == np.float64 and got.shape == (19,)
    assert np.array_equal(got, ref)
    mpl.save_npy_atomic(got, str(tmp_path / "mine.npy"))
    assert np.array_equal(np.load(tmp_path / "mine.npy"), ref)


def test_arguments():
    with pytest.raises(SystemExit):
        mpl.get_arguments(["--data-dir", "x"])                       # --restore-from is required
    a = mpl.get_arguments(["--restore-from", "m.pth"])
    assert a.arch == "multi" and a.input_size is None and a.label_size == (2048, 1024) and a.threshold is None
    assert a.eval_dtype == "f32" and a.num_workers == 8
    a = mpl.get_arguments(["--restore-from", "m.pth", "--arch", "single", "--input-size", "129,65", "--input-size", "161,81",
                           "--label-size", "321,161", "--threshold", "0.8", "--save-color"])
    assert a.input_size == [(129, 65), (161, 81)] and a.label_size == (321, 161) and a.threshold == 0.8 and a.save_color
    with pytest.raises(SystemExit):
        mpl.get_arguments(["--restore-from", "m.pth", "--model", "DeepLab"])     # --arch, not the reference scripts' --model
    with pytest.raises(SystemExit):
        mpl.get_arguments(["--restore-from", "m.pth", "--input-size", "1024x512"])


def test_bounded_map_keeps_order_and_bounds_the_queue():
    running, peak, lock = [0], [0], threading.Lock()
    started = []

    def fn(x):
        with lock:
            started.append(x)
            running[0] += 1
            peak[0] = max(peak[0], running[0])
        with lock:
            running[0] -= 1
        return x * x
    with ThreadPoolExecutor(4) as pool:
        it = mpl._bounded_map(pool, fn, range(100), 6)
        first = next(it)
        assert first == 0 and len(started) <= 7               # only `depth` (+1 refill) submitted ahead of the consumer
        rest = list(it)
    assert [first] + rest == [x * x for x in range(100)]


def test_train_class_dist_flag_checked_before_the_gpu(tmp_path):
    from simt_amd.tools import trainV2_simt as tool
    missing = str(tmp_path / "ClassDist_none.npy")
    with pytest.raises(SystemExit) as e:
        tool.main(["--synthetic", "--class-dist", missing, "--num-steps-stop", "1"])
    assert missing in str(e.value) and "does not exist" in str(e.value)
    np.save(tmp_path / "short.npy", np.full(18, 1 / 18))
    with pytest.raises(SystemExit, match=r"shape \(19,\)"):
        tool.main(["--synthetic", "--class-dist", str(tmp_path / "short.npy")])
    np.save(tmp_path / "unnorm.npy", np.full(19, 0.1))
    with pytest.raises(SystemExit, match="sum to 1"):
        tool.main(["--synthetic", "--class-dist", str(tmp_path / "unnorm.npy")])
    (tmp_path / "junk.npy").write_text("not an array")
    with pytest.raises(SystemExit, match="junk.npy"):
        tool.main(["--synthetic", "--class-dist", str(tmp_path / "junk.npy")])
    cd = mpl.class_dist(np.arange(1, 21), 19)
    np.save(tmp_path / "ok.npy", cd)
    assert np.array_equal(tool.load_class_dist_arg(str(tmp_path / "ok.npy"), 19), cd)
    assert tool.get_arguments([]).class_dist is None                     # without the flag: BAPA's prior, as before
