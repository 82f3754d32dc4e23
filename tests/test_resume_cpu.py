"""The host side of resuming a run (simt_amd/train_state.py, GpuLoader(start_batch=...), SnapshotKeeper.state, --train-state): position
arithmetic against brute-force iteration, the mirror generator's advance against actually drawing, the file round trip, the hash, the
hyper-parameter comparison, the rotation continued by a second keeper, the write cadence of the flag.  No GPU."""
import os
import types

import numpy as np
import pytest
import torch

from simt_amd import train_state as tsf
from simt_amd.data.pipeline import GpuLoader, loader_position, skip_mirror_draws
from simt_amd.step import Hyper
from simt_amd.tools.trainV2_simt import SnapshotKeeper, TrainStateFile, get_arguments


class _FakeDs:
    """What GpuLoader's host side asks of a dataset: len, decode(index), crop_size, is_mirror."""

    def __init__(self, n, mirror=True):
        self.n, self.is_mirror, self.crop_size, self.calls = n, mirror, (6, 4), []

    def __len__(self):
        return self.n

    def decode(self, i):
        self.calls.append(i)
        return np.full((4, 6, 3), i, np.uint8), np.full((4, 6), i, np.uint8), f"f{i}"


def _loader(ds, B, rank=0, world=1, seed=3, **kw):
    return GpuLoader(ds, B, shuffle=True, num_workers=2, seed=seed, rank=rank, world=world, **kw)


# ---- loader position ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items,B,rank,world", [(11, 2, 0, 1), (11, 2, 1, 2), (11, 2, 0, 2), (4, 2, 0, 1), (23, 4, 2, 3), (7, 7, 0, 1), (9, 1, 1, 4)])
def test_loader_position_equals_brute_force_iteration_of_order(n_items, B, rank, world):
    ld = _loader(_FakeDs(n_items), B, rank, world)
    brute = []
    for e in range(5):
        idx = ld._order(e)
        brute += [(e, b, idx[b * B:(b + 1) * B]) for b in range(len(idx) // B)]
    per_epoch = len(ld._order(0)) // B
    assert per_epoch > 0 and len(brute) == 5 * per_epoch
    for n, (e, b, _items) in enumerate(brute):
        assert loader_position(n_items, B, rank, world, n) == (e, b, per_epoch), n


def test_loader_position_refuses_what_cannot_be_reached():
    with pytest.raises(ValueError):
        loader_position(10, 2, 0, 1, -1)
    with pytest.raises(ValueError):
        loader_position(3, 2, 1, 2, 1)              # rank 1 of 2 holds one of three items: no batch of two, ever
    assert loader_position(3, 2, 1, 2, 0) == (0, 0, 0)


@pytest.mark.parametrize("n", [0, 1, 4, 5, 10, 13])
@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_host_batches_from_start_batch_are_the_tail_and_skip_no_decode(n, rank, world):
    """The host half of the loader on a fake dataset, 3 epochs: names and frames from start_batch = n on equal the default loader's tail;
    exactly the items of the yielded batches are decoded (n = 5: an epoch boundary for one rank, n = 10, 13: epoch 2)."""
    B = 2
    ds0 = _FakeDs(11)
    ref = [(rgb.copy(), meta[1]) for rgb, _lab, meta in _loader(ds0, B, rank, world, epochs=3)._host_batches()]
    per_epoch = len(range(rank, 11, world)) // B
    assert len(ref) == 3 * per_epoch
    ds1 = _FakeDs(11)
    got = [(rgb.copy(), meta[1]) for rgb, _lab, meta in _loader(ds1, B, rank, world, epochs=3, start_batch=n)._host_batches()]
    assert len(got) == max(0, len(ref) - n)
    for (ra, na), (rb, nb) in zip(ref[n:], got):
        assert na == nb and np.array_equal(ra, rb)
    assert sorted(ds1.calls) == sorted(int(name[1:]) for _r, names in ref[n:] for name in names)


# ---- mirror draws -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n", [(1, 0), (1, 7), (2, 5), (3, 4), (4, 1000)])
def test_skip_mirror_draws_equals_drawing(B, n):
    a = np.random.default_rng(99)
    drawn = [(a.integers(0, 2, B) == 0).tolist() for _ in range(n + 4)]
    b = skip_mirror_draws(np.random.default_rng(99), B, n)
    assert [(b.integers(0, 2, B) == 0).tolist() for _ in range(4)] == drawn[n:]


def test_loader_advances_its_mirror_generator_only_for_a_mirroring_dataset():
    B, n, seed, rank = 2, 5, 3, 1
    ld = _loader(_FakeDs(11, mirror=True), B, rank, 2, seed=seed, start_batch=n)
    ref = skip_mirror_draws(np.random.default_rng(seed + 7919 * rank), B, n)
    assert ld._rng.integers(0, 2, 8).tolist() == ref.integers(0, 2, 8).tolist()
    ld = _loader(_FakeDs(11, mirror=False), B, rank, 2, seed=seed, start_batch=n)
    assert ld._rng.integers(0, 2, 8).tolist() == np.random.default_rng(seed + 7919 * rank).integers(0, 2, 8).tolist()


# ---- the file -----------------------------------------------------------------------------------------------------------------------------
def _hand_made():
    g = torch.Generator().manual_seed(1)
    return {"model": {"a.weight": torch.randn(3, 2, generator=g), "a.num_batches_tracked": torch.tensor(7)},
            "momentum": {"a.weight": torch.randn(3, 2, generator=g)}, "ntm": [torch.randn(4, 2, generator=g), torch.randn(4, 2, generator=g)],
            "it_done": 7, "bad_reported": 2, "hyper": {"lr": 2.5e-4, "arch": {"layers": [1, 1, 2, 1]}, "format_version": tsf.FORMAT_VERSION},
            "accumulators": {"lout": torch.arange(16.0)}, "frozen_sha256": "ab" * 32}


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b and type(a) is type(b)


def test_save_load_round_trip_and_a_truncated_tmp_is_ignored(tmp_path):
    path = str(tmp_path / "run.state")
    ts, ks, ls = _hand_made(), {"best_mIoU": 41.5, "best_iter": 2000, "rolling_iter": None}, {"world": 1}
    tsf.save(path, ts, ks, ls)
    assert os.listdir(tmp_path) == ["run.state"]                   # the temporary name is gone
    good = open(path, "rb").read()
    open(path + ".tmp", "wb").write(good[:len(good) // 3])         # a later write that died a third of the way through
    ts2, ks2, ls2 = tsf.load(path)
    assert _same(ts, ts2) and ks2 == ks and ls2 == ls
    with pytest.raises(Exception):
        tsf.load(path + ".tmp")
    tsf.save(path, ts, None, None)                                  # the next write replaces both
    assert os.listdir(tmp_path) == ["run.state"] and tsf.load(path)[1:] == (None, {})


def test_load_refuses_a_snapshot_and_another_format_version(tmp_path):
    snap = str(tmp_path / "GTA5_5.pth")
    torch.save({"conv1.weight": torch.zeros(2)}, snap)
    with pytest.raises(ValueError, match="not a train-state file"):
        tsf.load(snap)
    torch.save({"format_version": tsf.FORMAT_VERSION + 1, "trainer": {}}, snap)
    with pytest.raises(ValueError, match="format_version"):
        tsf.load(snap)


def test_transition_parameters_reads_the_ntms_of_a_state_file(tmp_path):
    path = str(tmp_path / "s")
    ts = _hand_made()
    ts["wraw"] = [torch.ones(4, 4), torch.zeros(4, 4)]
    tsf.save(path, ts, None, None)
    tp = tsf.transition_parameters(path)
    assert _same(tp, {"ntm": ts["ntm"], "wraw": ts["wraw"]})
    del ts["ntm"]
    ts["hyper"]["trainer"] = "WarmupTrainer"
    tsf.save(path, ts, None, None)
    with pytest.raises(ValueError, match="WarmupTrainer"):
        tsf.transition_parameters(path)


# ---- the hash -----------------------------------------------------------------------------------------------------------------------------
def test_state_sha256_ignores_dict_order_and_sees_one_element():
    g = torch.Generator().manual_seed(5)
    st = {"b.weight": torch.randn(4, 3, 2, generator=g), "a.bias": torch.randn(5, generator=g), "a.num_batches_tracked": torch.tensor(3),
          "c.weight": torch.randn(2, 2, generator=g).t()}      # (one non-contiguous tensor)
    h = tsf.state_sha256(st)
    assert len(h) == 64 and h == tsf.state_sha256(dict(reversed(list(st.items())))) == tsf.state_sha256({k: v.clone() for k, v in st.items()})
    for k in st:
        other = {n: v.clone() for n, v in st.items()}
        flat = other[k].reshape(-1) if other[k].is_contiguous() else None
        if flat is None:
            other[k] = other[k].contiguous()
            flat = other[k].reshape(-1)
        flat[-1] = flat[-1] + 1
        assert tsf.state_sha256(other) != h, k
    renamed = {("z" + k if k == "a.bias" else k): v for k, v in st.items()}
    assert tsf.state_sha256(renamed) != h
    assert tsf.state_sha256({"a": torch.zeros(6)}) != tsf.state_sha256({"a": torch.zeros(2, 3)})


# ---- the hyper-parameter comparison -------------------------------------------------------------------------------------------------------
def _hyper(**kw):
    hp = {k: v for k, v in Hyper(**{k: v for k, v in kw.items() if k in Hyper().__dict__}).__dict__.items()}
    hp.update(B=2, H=65, W=129, dtype="bf16", trainer="SimTTrainer", model="v2", arch={"layers": [3, 4, 23, 3]}, format_version=tsf.FORMAT_VERSION)
    hp.update({k: v for k, v in kw.items() if k not in Hyper().__dict__})
    return hp


def test_hyper_mismatches_names_exactly_the_differing_fields():
    base = _hyper()
    assert tsf.hyper_mismatches(base, _hyper()) == []
    changed = dict(lr=1e-3, lr_T=1e-2, momentum=0.8, weight_decay=1e-4, power=0.8, num_steps=1000, lambda_seg=0.2, lambda_place=0.2,
                   lambda_convex=0.4, lambda_volume=0.2, lambda_anchor=0.4, th_high=0.9, th_low=0.1, num_classes=18, open_classes=3, iter_size=2,
                   B=4, H=64, W=128, dtype="f32", trainer="WarmupTrainer", model="v3", arch={"layers": [3, 4, 6, 3]},
                   format_version=tsf.FORMAT_VERSION + 1)
    assert set(changed) == set(tsf.CHECKED_FIELDS)
    for f, v in changed.items():
        assert tsf.hyper_mismatches(base, _hyper(**{f: v})) == [f]
    assert tsf.hyper_mismatches(base, _hyper(lr=1e-3, W=128, open_classes=3)) == ["lr", "open_classes", "W"]
    # a file round trip may turn tuples into lists: not a difference
    assert tsf.hyper_mismatches(base, _hyper(arch={"layers": (3, 4, 23, 3)})) == []
    # a field missing on one side is a difference
    short = dict(base)
    del short["th_low"]
    assert tsf.hyper_mismatches(short, base) == ["th_low"]


def test_hyper_mismatches_ignores_what_may_differ_between_the_two_commands():
    base = _hyper()
    free = _hyper(skip_unapplied_grads=True, num_steps_stop=6, save_pred_every=7, print_every=3, num_workers=9, cache_dataset="device")
    assert free != base and tsf.hyper_mismatches(base, free) == []


# ---- the snapshot rotation ----------------------------------------------------------------------------------------------------------------
def test_snapshot_keeper_state_continues_a_rotation(tmp_path, capsys):
    sd = {"w": torch.ones(2)}
    k1 = SnapshotKeeper(str(tmp_path), "GTA5_iter")
    assert k1.state() == {"best_mIoU": 0, "best_iter": 0, "rolling_iter": None}
    k1.rolling(sd, 2)
    k1.best(sd, 2, 31.25)
    assert sorted(os.listdir(tmp_path)) == ["GTA5_iter2.pth", "GTA5_iter2_mIoU31.25.pth"]
    st = k1.state()
    # a keeper that knows nothing leaves the superseded files behind ...
    k0 = SnapshotKeeper(str(tmp_path / "x"), "GTA5_iter")
    os.makedirs(k0.dir)
    k0.rolling(sd, 4)
    # ... the resumed one removes them
    k2 = SnapshotKeeper(str(tmp_path), "GTA5_iter")
    k2.load_state(st)
    assert k2.state() == st
    k2.rolling(sd, 4)
    assert sorted(os.listdir(tmp_path)) == ["GTA5_iter2_mIoU31.25.pth", "GTA5_iter4.pth", "x"]
    assert not k2.best(sd, 4, 30.0)                                  # not better than the best of the run it continues
    assert k2.best(sd, 6, 33.5)
    assert sorted(os.listdir(tmp_path)) == ["GTA5_iter4.pth", "GTA5_iter6_mIoU33.5.pth", "x"]
    capsys.readouterr()


# ---- the flag -----------------------------------------------------------------------------------------------------------------------------
class _FakeTrainer:
    def __init__(self):
        self.it_done, self.loaded = 0, None

    def training_state(self):
        return {"it_done": self.it_done, "hyper": {}}

    def load_training_state(self, ts):
        if ts["it_done"] == 13:
            raise ValueError("lr (state: 1, this trainer: 2)")
        self.loaded, self.it_done = ts, ts["it_done"]

    def state_dict(self):
        return {"w": torch.zeros(1)}


def _flag(tmp_path, *extra):
    args = get_arguments(["--snapshot-dir", str(tmp_path), "--save-pred-every", "4"] + list(extra))
    return TrainStateFile(args, 0, 1), args


def _written_at(tmp_path, rf, n):
    tr, keeper, path, out = _FakeTrainer(), SnapshotKeeper(str(tmp_path), "GTA5_iter"), rf.path, []
    for i in range(n):
        tr.it_done = i + 1
        if os.path.exists(path):
            os.remove(path)
        rf.after_iteration(i, tr, keeper)
        if os.path.exists(path):
            assert tsf.load(path)[0]["it_done"] == i + 1
            out.append(i)
    return out


def test_train_state_flag_write_cadence_and_defaults(tmp_path):
    args = get_arguments([])
    assert args.train_state is None and args.train_state_every is None
    off, _ = _flag(tmp_path)
    tr, keeper = _FakeTrainer(), SnapshotKeeper(str(tmp_path), "GTA5_iter")
    assert off.resume(tr, keeper) == 0 and not off.complete(0, 5, tr, str(tmp_path))
    off.after_iteration(4, tr, keeper)
    off.write(tr, keeper)
    assert os.listdir(tmp_path) == []                                # without the flag: nothing
    f = str(tmp_path / "run.state")
    rf, _ = _flag(tmp_path, "--train-state", f)
    assert _written_at(tmp_path, rf, 13) == [4, 8, 12]               # the loop's snapshot decision: i % save_pred_every == 0 and i != 0
    rf, _ = _flag(tmp_path, "--train-state", f, "--train-state-every", "5")
    assert _written_at(tmp_path, rf, 13) == [4, 9]                   # every 5 iterations: after the 5th and the 10th
    with pytest.raises(SystemExit):
        _flag(tmp_path, "--train-state-every", "5")
    with pytest.raises(SystemExit):
        _flag(tmp_path, "--train-state", f, "--train-state-every", "0")
    # rank 1 never writes
    args = get_arguments(["--train-state", f, "--save-pred-every", "1"])
    assert not os.path.exists(f)
    TrainStateFile(args, 1, 2).write(tr, keeper)
    assert not os.path.exists(f)


def test_train_state_flag_resume_complete_and_refusals(tmp_path, capsys):
    f = str(tmp_path / "run.state")
    rf, _ = _flag(tmp_path, "--train-state", f)
    tr, keeper = _FakeTrainer(), SnapshotKeeper(str(tmp_path), "GTA5_iter")
    assert rf.resume(tr, keeper) == 0 and tr.loaded is None          # FILE does not exist: a fresh run
    tr.it_done = 6
    keeper.rolling_iter = 4
    rf.write(tr, keeper)
    tr2, keeper2 = _FakeTrainer(), SnapshotKeeper(str(tmp_path), "GTA5_iter")
    assert rf.resume(tr2, keeper2) == 6 and keeper2.rolling_iter == 4
    assert "resumed _FakeTrainer from" in capsys.readouterr().out
    assert not rf.complete(6, 7, tr2, str(tmp_path))
    assert rf.complete(6, 6, tr2, str(tmp_path)) and os.path.exists(tmp_path / "GTA5_6.pth")
    assert "complete" in capsys.readouterr().out
    before = os.path.getmtime(tmp_path / "GTA5_6.pth")
    assert rf.complete(7, 6, tr2, str(tmp_path)) and os.path.getmtime(tmp_path / "GTA5_6.pth") == before      # an existing final snapshot stays
    # written over 1 GPU, resumed over 2; and a trainer that refuses the state
    with pytest.raises(SystemExit, match="1 GPU"):
        TrainStateFile(types.SimpleNamespace(train_state=f, train_state_every=None, save_pred_every=4), 0, 2).resume(tr2, keeper2)
    tr.it_done = 13
    rf.write(tr, keeper)
    with pytest.raises(SystemExit, match="lr"):
        rf.resume(_FakeTrainer(), keeper2)


def test_train_state_flag_refuses_another_seed_mirror_data_list_or_class_prior(tmp_path, capsys):
    """What the loop feeds the trainer travels in the file too: re-issuing the command with another --random-seed, --random-mirror, data list
    or class prior is another run.  What may differ (--num-steps-stop, --save-pred-every, --print-every, --num-workers, --cache-dataset) is not."""
    f, lst = str(tmp_path / "run.state"), tmp_path / "pseudo.lst"
    lst.write_text("a.png b.png\n")
    cd = np.full(19, 1 / 19, np.float32)
    base = ["--train-state", f, "--snapshot-dir", str(tmp_path), "--data-list-target", str(lst)]

    def flag(extra=(), prior=cd):
        return TrainStateFile(get_arguments(base + list(extra)), 0, 1, prior)
    tr, keeper = _FakeTrainer(), SnapshotKeeper(str(tmp_path), "GTA5_iter")
    tr.it_done = 3
    first = flag()
    first.write(tr, keeper)
    assert set(tsf.load(f)[2]["run"]) == {"random_seed", "random_mirror", "synthetic", "class_dist_sha256", "data_list_sha256"}
    assert flag(["--num-steps-stop", "9", "--save-pred-every", "7", "--print-every", "3", "--num-workers", "1", "--cache-dataset", "device"]
                ).resume(_FakeTrainer(), keeper) == 3
    for extra, prior, name in ((["--random-seed", "5"], cd, "random_seed"), (["--random-mirror"], cd, "random_mirror"),
                               (["--synthetic"], cd, "synthetic"), ([], np.roll(np.linspace(0.01, 0.09, 19, dtype=np.float32), 1), "class_dist_sha256")):
        with pytest.raises(SystemExit, match=name) as e:
            flag(extra, prior).resume(_FakeTrainer(), keeper)
        assert sum(k in str(e.value) for k in first.run) == 1, str(e.value)          # exactly the differing one is named
    lst.write_text("a.png b.png\nc.png d.png\n")
    with pytest.raises(SystemExit, match="data_list_sha256"):
        flag().resume(_FakeTrainer(), keeper)
    capsys.readouterr()


def test_save_atomic_lives_in_the_library_and_the_tools_re_export_it():
    from simt_amd.tools import trainV1_warmup, trainV2_simt
    assert trainV2_simt.save_atomic is tsf.save_atomic is trainV1_warmup.save_atomic
