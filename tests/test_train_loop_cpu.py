"""The outer loop both training tools share (simt_amd/tools/train_loop.py: `train`), driven by a stub trainer that records its calls: which
iterations step, print, snapshot, evaluate and write the train state, on rank 0 and beside it, from a fresh start and from a resumed one."""
import os
import re
import types

import pytest
import torch

from simt_amd.tools import train_loop, trainV2_simt


class _Trainer:
    ema = None

    def __init__(self, log):
        self.log, self.params = log, {"w": torch.zeros(1)}

    def step(self, img, lab, i_iter, **kw):
        self.log.append(("step", i_iter, img, lab, kw))

    def losses(self):
        self.log.append(("losses", self.log[-1][1]))
        return {"loss": 0.5}

    def state_dict(self):
        return {"w": torch.full((1,), float(self.log[-1][1]))}


def _args(tmp_path, **kw):
    a = dict(snapshot_dir=str(tmp_path), num_steps=7, num_steps_stop=6, print_every=2, save_pred_every=2, data_dir_val="", iter_size=1,
             batch_size=2, train_state=None, train_state_every=None)
    a.update(kw)
    return types.SimpleNamespace(**a)


def _run(args, log, rank=0, world=1, make_score=None):
    """train() over the stub: open_data logs its start batch, next_step its call; the loss line is `<i> <rate>`."""
    def open_data(start_batch):
        log.append(("open", start_batch))
        return lambda: (("img", "lab"), {"k": len(log)})
    train_loop.train(args, _Trainer(log), "GTA5_iter", None, rank, world, open_data, lambda i, l, rate: f"line {i} {l['loss']} {rate!r}",
                     make_score or (lambda: pytest.fail("no evaluation without --data-dir-val")))
    return [e[1] for e in log if e[0] == "step"], [e[1] for e in log if e[0] == "losses"]


@pytest.fixture
def spies(monkeypatch):
    """after_iteration and shutdown recorded (the real ones still run where they can: shutdown would need a process group)."""
    seen = {"after": [], "shutdown": [], "rolling": []}
    real_after, real_rolling = trainV2_simt.TrainStateFile.after_iteration, trainV2_simt.SnapshotKeeper.rolling
    monkeypatch.setattr(trainV2_simt.TrainStateFile, "after_iteration",
                        lambda self, i, tr, keeper: (seen["after"].append(i), real_after(self, i, tr, keeper))[1])
    monkeypatch.setattr(trainV2_simt.SnapshotKeeper, "rolling",
                        lambda self, sd, i: (seen["rolling"].append(i), real_rolling(self, sd, i))[1])
    monkeypatch.setattr(train_loop, "shutdown", lambda world: seen["shutdown"].append(world))
    monkeypatch.setattr(torch.distributed, "init_process_group", lambda *a, **k: pytest.fail("the loop creates no process group"), raising=False)
    return seen


def test_no_validation_directory_rank0(tmp_path, capsys, spies):
    log = []
    steps, losses = _run(_args(tmp_path), log)
    assert steps == [0, 1, 2, 3, 4, 5] and losses == [0, 2, 4]
    assert log[0] == ("open", 0) and all(e[2:] == ("img", "lab", {"k": n}) for n, e in enumerate(log) if e[0] == "step")
    assert spies["rolling"] == [2, 4] and spies["after"] == [0, 1, 2, 3, 4] and spies["shutdown"] == [1]
    assert sorted(os.listdir(tmp_path)) == ["GTA5_6.pth", "GTA5_iter4.pth"]          # the rotation removed GTA5_iter2.pth
    assert torch.load(tmp_path / "GTA5_6.pth")["w"].item() == 5.0                      # written at i = 5
    out = capsys.readouterr().out.splitlines()
    assert [ln.split()[:3] for ln in out] == [["line", "0", "0.5"], ["line", "2", "0.5"], ["line", "4", "0.5"], ["save", "model", "..."]]


def test_no_validation_directory_rank1_of_2(tmp_path, capsys, spies):
    log = []
    steps, losses = _run(_args(tmp_path), log, rank=1, world=2)
    assert steps == [0, 1, 2, 3, 4, 5] and losses == [0, 2, 4]           # a bad-label error is raised on every rank
    assert capsys.readouterr().out == "" and os.listdir(tmp_path) == [] and spies["rolling"] == []
    assert spies["after"] == [0, 1, 2, 3, 4] and spies["shutdown"] == [2]


@pytest.mark.parametrize("rank", [0, 1])
def test_validation_directory(tmp_path, capsys, spies, monkeypatch, rank):
    log, built, scored, best = [], [], [], []
    real_best = trainV2_simt.SnapshotKeeper.best
    monkeypatch.setattr(trainV2_simt.SnapshotKeeper, "best", lambda self, sd, i, m: (best.append((i, m)), real_best(self, sd, i, m))[1])

    def make_score():
        built.append(len(log))
        return lambda params: (scored.append((log[-1][1], params)), 10.0 * log[-1][1] + 0.25)[1]
    steps, losses = _run(_args(tmp_path, data_dir_val="val"), log, rank=rank, world=2, make_score=make_score)
    assert steps == [0, 1, 2, 3, 4, 5] and losses == [0, 2, 4]
    assert len(built) == 1 and [i for i, _p in scored] == [2, 4] and all(p == {"w": torch.zeros(1)} for _i, p in scored)
    assert spies["rolling"] == [] and spies["after"] == [0, 1, 2, 3, 4]
    out = capsys.readouterr().out
    if rank == 0:
        assert best == [(2, 20.25), (4, 40.25)]
        assert sorted(os.listdir(tmp_path)) == ["GTA5_6.pth", "GTA5_iter4_mIoU40.25.pth"]
        assert len(re.findall(r"Begin evaluation on iter", out)) == 2 and out.count("Finish Evaluation: ") == 2
    else:
        assert best == [] and os.listdir(tmp_path) == [] and out == ""


def test_start_at_3(tmp_path, capsys, spies, monkeypatch):
    log, clock = [], iter([100.0, 104.0, 110.0])
    monkeypatch.setattr(trainV2_simt.TrainStateFile, "resume", lambda self, tr, keeper: 3)
    monkeypatch.setattr(train_loop, "time", types.SimpleNamespace(time=lambda: next(clock)))      # the loop's clock only
    steps, losses = _run(_args(tmp_path, iter_size=2, print_every=1, num_steps_stop=5), log)
    assert log[0] == ("open", 6) and steps == [3, 4] and losses == [3, 4]
    out = capsys.readouterr().out.splitlines()
    # batch 2 x 1 GPU x (i_iter + 1 - start) images over the seconds since the loop began
    assert out[:2] == [f"line 3 0.5 {2 * 1 * 1 / 4.0!r}", f"line 4 0.5 {2 * 1 * 2 / 10.0!r}"]


def test_complete_run_only_shuts_down(tmp_path, capsys, spies, monkeypatch):
    log = []
    monkeypatch.setattr(trainV2_simt.TrainStateFile, "resume", lambda self, tr, keeper: 6)
    monkeypatch.setattr(trainV2_simt.TrainStateFile, "complete", lambda self, start, stop, tr, d: (log.append(("complete", start, stop)), True)[1])
    steps, losses = _run(_args(tmp_path), log)
    assert log == [("complete", 6, 6)] and steps == [] and losses == [] and spies["shutdown"] == [1] and spies["after"] == []
