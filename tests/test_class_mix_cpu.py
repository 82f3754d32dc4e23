"""Host side of --class-mix (simt_amd/data/class_mix.py, the tools' flag, the descriptor's layout, the restatement's own properties): no
GPU needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _class_mix_ref as ref
from simt_amd.data import class_mix as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "simt_hip.h")).read()


def test_header_declares_the_symbols_and_the_descriptor_matches_ctypes():
    """sizeof / offsetof of simt_class_mix_desc from a compiled C program against the ctypes mirror; symbols added, the ABI version stays."""
    from simt_amd import _lib as L
    assert re.search(r"int\s+simt_label_presence\s*\(", HDR) and re.search(r"int\s+simt_class_mix\s*\(", HDR)
    assert L.ABI_VERSION == 2 and int(re.search(r"#define\s+SIMT_ABI_VERSION\s+(\d+)", HDR).group(1)) == 2
    fields = [n for n, _t in L.ClassMixDesc._fields_]
    assert fields == ["x", "lab", "x_out", "lab_out", "part", "B", "h", "w", "n_classes", "partner", "apply", "rank"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "simt_hip.h"\nint main(void){'
           'printf("size %zu\\n", sizeof(simt_class_mix_desc));' +
           "".join(f'printf("{n} %zu\\n", offsetof(simt_class_mix_desc, {n}));' for n in fields) +
           'printf("max %d %d %d\\n", SIMT_CLASS_MIX_MAX, SIMT_CLASS_MIX_CLASSES, SIMT_CLASS_MIX_PARTS);return 0;}')
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", exe])
        out = dict(ln.split(None, 1) for ln in subprocess.check_output([exe]).decode().splitlines())
    assert C.sizeof(L.ClassMixDesc) == int(out["size"]) < 4096          # it travels as kernel arguments
    for n in fields:
        assert getattr(L.ClassMixDesc, n).offset == int(out[n]), n
    assert out["max"].split() == [str(L.CLASS_MIX_MAX), str(L.CLASS_MIX_CLASSES), str(L.CLASS_MIX_PARTS)] == ["32", "32", "64"]
    assert (cm.MAX_ITEMS, cm.MAX_CLASSES) == (L.CLASS_MIX_MAX, L.CLASS_MIX_CLASSES)
    assert "simt_label_presence" in L.SIGNATURES and "simt_class_mix" in L.SIGNATURES


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_draws_are_deterministic_per_seed_and_rank_and_equal_the_documented_order():
    B, Cn = 4, 19
    a = [cm.draw_batch(g, B, Cn, 0.5) for g in [cm.generator(7, 0)] for _ in range(3)]
    b = [cm.draw_batch(g, B, Cn, 0.5) for g in [cm.generator(7, 0)] for _ in range(3)]
    c = [cm.draw_batch(g, B, Cn, 0.5) for g in [cm.generator(7, 1)] for _ in range(3)]
    d = [ref.draws(g, B, Cn, 0.5) for g in [ref.generator(7, 0)] for _ in range(3)]
    assert all(_same(p, q) for p, q in zip(a, b)) and all(_same(p, q) for p, q in zip(a, d))
    assert not any(np.array_equal(p[1], q[1]) for p, q in zip(a, c)), "ranks 0 and 1 drew the same permutations"
    assert not _same(cm.draw_batch(cm.generator(8, 0), B, Cn, 0.5), a[0])
    for apply, rank in a + c:
        assert apply.dtype == np.bool_ and apply.shape == (B,) and rank.dtype == np.uint8 and rank.shape == (B, Cn)
        for row in rank:
            assert sorted(row.tolist()) == list(range(Cn))
    # the generator is not the loader's: the loader's stream for the same seed gives other numbers
    assert not np.array_equal(np.random.default_rng(7).random(B), cm.generator(7, 0).random(B))


@pytest.mark.parametrize("prob", [1.0, 0.3])
def test_skipping_equals_consuming_the_draws(prob):
    B, Cn = 3, 19
    for n in (0, 1, 5):
        a, b = cm.generator(11, 2), cm.generator(11, 2)
        for _ in range(n):
            cm.draw_batch(a, B, Cn, prob)
        cm.skip_draws(b, B, n, Cn)
        assert a.bit_generator.state == b.bit_generator.state
        assert _same(cm.draw_batch(a, B, Cn, prob), cm.draw_batch(b, B, Cn, prob))
    # both draws are made whatever prob is: the stream position after a batch does not depend on it
    a, b = cm.generator(11, 2), cm.generator(11, 2)
    cm.draw_batch(a, B, Cn, 1.0)
    cm.draw_batch(b, B, Cn, 0.3)
    assert a.bit_generator.state == b.bit_generator.state
    assert cm.draw_batch(cm.generator(1, 0), B, Cn, 1.0)[0].all()


def _random_case(rng):
    B = int(rng.integers(2, 5))
    Cn = int(rng.integers(1, 33))
    h, w = int(rng.integers(1, 9)), int(rng.integers(1, 9))
    pool = rng.choice(Cn, size=int(rng.integers(1, Cn + 1)), replace=False)
    lab = rng.choice(np.concatenate([pool, [255, Cn + 1, -1]]), size=(B, h, w)).astype(np.int64)
    if rng.random() < 0.2:
        lab[int(rng.integers(0, B))] = 255
    x = rng.integers(-2 ** 31, 2 ** 31, (B, 3, h, w), dtype=np.int64).astype(np.int32)
    apply = rng.random(B) < 0.7
    rank = rng.permuted(np.tile(np.arange(Cn, dtype=np.uint8), (B, 1)), axis=1)
    return B, Cn, x, lab, apply, rank


def test_restatement_properties_over_200_random_cases():
    rng = np.random.default_rng(2021)
    seen_empty = seen_odd = 0
    for _ in range(200):
        B, Cn, x, lab, apply, rank = _random_case(rng)
        m = ref.paste_masks(lab, apply, rank, Cn)
        xo, lo = ref.mix(x, lab, apply, rank, Cn)
        for i in range(B):
            j = (i + 1) % B
            P, S = ref.present(lab[j], Cn), ref.chosen(lab[j], rank[i], Cn)
            n = len(P)
            assert len(S) == -(-n // 2) and S <= P                                   # ceil(n / 2), a subset of the present classes
            assert all(rank[i][c] < rank[i][o] for c in S for o in P - S)            # the smallest ranks
            seen_empty += n == 0
            seen_odd += n % 2
            if not apply[i] or n == 0:                                                # the identity
                assert not m[i].any() and np.array_equal(xo[i], x[i]) and np.array_equal(lo[i], lab[i])
                continue
            pasted = lab[j][m[i]]
            assert ((pasted >= 0) & (pasted < Cn)).all() and set(pasted.tolist()) == S      # no ignore pixel; every chosen class, whole
            assert np.array_equal(lo[i][m[i]], pasted) and np.array_equal(lo[i][~m[i]], lab[i][~m[i]])
            for ch in range(3):
                assert np.array_equal(xo[i, ch][m[i]], x[j, ch][m[i]]) and np.array_equal(xo[i, ch][~m[i]], x[i, ch][~m[i]])
    assert seen_empty > 0 and seen_odd > 0


def test_parse_refuses_bad_values_and_names_them():
    assert cm.parse("1.0", 19, 2) == (19, 1.0) and cm.parse(0.25, 32, 32) == (32, 0.25) and cm.parse("1", 1, 2) == (1, 1.0)
    for value, Cn, B, named in [("0", 19, 2, r"--class-mix '0'"), ("1.5", 19, 2, r"--class-mix '1\.5'"), ("x", 19, 2, r"--class-mix 'x'"),
                                ("nan", 19, 2, r"--class-mix 'nan'"), ("1.0", 33, 2, r"--class-mix with 33 classes"),
                                ("1.0", 19, 1, r"--class-mix with a batch of 1\b"), ("1.0", 19, 33, r"--class-mix with a batch of 33\b")]:
        with pytest.raises(ValueError, match=named):
            cm.parse(value, Cn, B)


def _args(tool, *extra):
    return tool.get_arguments(list(extra))


def test_cli_parses_the_flag_on_both_tools_and_exits_on_bad_values():
    from simt_amd.tools import trainV1_warmup, trainV2_simt
    for tool in (trainV1_warmup, trainV2_simt):
        a = _args(tool)
        assert a.class_mix is None and trainV2_simt.class_mix_setting(a) is None
        assert trainV2_simt.class_mix_setting(_args(tool, "--class-mix", "--batch-size", "2")) == (19, 1.0)
        assert trainV2_simt.class_mix_setting(_args(tool, "--class-mix", "0.5", "--batch-size", "4", "--num-classes", "7")) == (7, 0.5)
        for extra, named in [(["--class-mix"], r"batch of 1\b"), (["--class-mix", "--batch-size", "33"], r"batch of 33\b"),
                             (["--class-mix", "0", "--batch-size", "2"], r"--class-mix '0'"),
                             (["--class-mix", "1.5", "--batch-size", "2"], r"--class-mix '1\.5'"),
                             (["--class-mix", "--batch-size", "2", "--num-classes", "33"], r"33 classes")]:
            with pytest.raises(SystemExit, match=named):
                trainV2_simt.class_mix_setting(_args(tool, *extra))


def test_synthetic_says_once_that_the_flag_does_nothing(capsys):
    from simt_amd.tools import trainV2_simt as tool
    cd = np.full(19, 1 / 19, np.float32)
    assert tool.batches(_args(tool, "--synthetic", "--class-mix", "0.5", "--batch-size", "2"), 2, 8, 8, cd, 0, 1, "cpu") is not None
    assert "--class-mix does nothing with --synthetic" in capsys.readouterr().out
    tool.batches(_args(tool, "--synthetic"), 1, 8, 8, cd, 0, 1, "cpu")
    assert "class-mix" not in capsys.readouterr().out


def test_run_identity_holds_the_probability_and_a_resume_that_differs_is_refused(tmp_path):
    import torch

    from simt_amd import train_state
    from simt_amd.tools import trainV2_simt as tool
    cd = np.full(19, 1 / 19, np.float32)
    lst = tmp_path / "list.lst"
    lst.write_text("a b\n")
    base = ["--data-list-target", str(lst), "--batch-size", "2"]
    off = tool.run_identity(_args(tool, *base), cd)
    on = tool.run_identity(_args(tool, *base, "--class-mix", "0.5"), cd)
    assert "class_mix" not in off and tool.RUN_DEFAULTS["class_mix"] is False and on["class_mix"] == 0.5          # absent = False
    assert tool.run_identity(_args(tool, *base, "--class-mix"), cd)["class_mix"] == 1.0
    assert {k: v for k, v in on.items() if k != "class_mix"} == off
    assert "class_mix" not in tool.run_identity(_args(tool, *base, "--class-mix", "0.5", "--synthetic"), cd)      # it does nothing there

    class Tr:
        it_done = 0

        def load_training_state(self, ts):
            self.it_done = ts["it_done"]

    keeper = tool.SnapshotKeeper(str(tmp_path), "x")
    path = str(tmp_path / "run.state")
    train_state.save(path, {"it_done": 3, "w": torch.zeros(1)}, keeper.state(), {"world": 1, "run": on})
    assert tool.TrainStateFile(_args(tool, *base, "--class-mix", "0.5", "--train-state", path), 0, 1, cd).resume(Tr(), keeper) == 3
    for other in (["--class-mix", "0.25"], ["--class-mix"], []):
        with pytest.raises(SystemExit, match=r"differs in: class_mix \(state: 0\.5"):
            tool.TrainStateFile(_args(tool, *base, *other, "--train-state", path), 0, 1, cd).resume(Tr(), keeper)
    # a state file from before the key existed lacks it and still loads with the flag off: it is the state of a run without the mix
    train_state.save(path, {"it_done": 2, "w": torch.zeros(1)}, keeper.state(), {"world": 1, "run": off})
    assert tool.TrainStateFile(_args(tool, *base, "--train-state", path), 0, 1, cd).resume(Tr(), keeper) == 2
    with pytest.raises(SystemExit, match=r"differs in: class_mix \(state: False, this run: 1\.0"):
        tool.TrainStateFile(_args(tool, *base, "--class-mix", "--train-state", path), 0, 1, cd).resume(Tr(), keeper)


def test_dataset_stores_the_pair_like_scale_crop(tmp_path):
    from simt_amd.dataset.cityscapes_dataset import cityscapesPseudo
    lst = tmp_path / "l.lst"
    lst.write_text("a.png b.png\n")
    assert cityscapesPseudo(str(tmp_path), str(lst)).class_mix is None
    assert cityscapesPseudo(str(tmp_path), str(lst), class_mix=(19, "0.5")).class_mix == (19, 0.5)
