#!/usr/bin/env python3
"""Cost of a train-state write (simt_amd/train_state.py) -> profiles/train_state.txt.

    python profiles/tools/train_state_cost.py [--out FILE] [--pairs 3] [--steps 200] [--every 50]

Full-depth DeepLab-v2 SimT trainer at the benchmark's size (B = 4, 768 x 768, bf16, K = 3).
  1. one write: save_atomic(tr.state_dict()) (the snapshot the tools always wrote) alternating with training_state() + train_state.save,
     file sizes, the way back (load + load_training_state), the SHA-256 of the frozen model.
  2. step rate with and without the writes, the trainer's own loop on ONE resident batch (no input cost): a warm-up run that is thrown
     away, then `--pairs` pairs in alternating order (off, on, on, off, ...), `--steps` steps each, a write every `--every` steps through
     the tools' TrainStateFile; wall time from a synchronised start to a synchronised end.
  3. the same through `trainV2_simt --synthetic` (its batches are built on the host every step): warm-up run, alternating pairs, the
     images/s the tool prints at its last iteration.
"""
import argparse
import contextlib
import io
import os
import re
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from simt_amd import model_spec as ms  # noqa: E402
from simt_amd import train_state  # noqa: E402
from simt_amd.step import Hyper, SimTTrainer  # noqa: E402
from simt_amd.tools import trainV2_simt as tool  # noqa: E402

K, B, H, W = 3, 4, 768, 768


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--every", type=int, default=50)
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None

    def say(*s):
        print(*s, flush=True)
        if out:
            print(*s, file=out, flush=True)

    dev = torch.device("cuda:0")
    cd = ms.load_class_dist("bapa")
    st = ms.trained_like_init(ms.state_shapes(19, K, True), seed=1234)
    fst = ms.trained_like_init(ms.state_shapes(19, 0, False), seed=1234)

    def trainer():
        return SimTTrainer(st, fst, ms.ntm_init(19, K, 1), ms.ntm_init(19, K, 2), Hyper(open_classes=K, lr=6e-4, lr_T=6e-3), cd, B, H, W,
                           dtype=torch.bfloat16, device=dev)
    t = time.time()
    tr = trainer()
    tc = time.time() - t
    t = time.time()
    train_state.state_sha256(tr.fixed_params)
    say(f"trainer construction {tc:.2f} s, of it the SHA-256 of the frozen model {time.time() - t:.3f} s")
    img, lab = ms.synthetic_batch(B, H, W, cd, seed=5, device=dev)
    for _ in range(3):
        tr.step(img, lab)
    tr.losses()
    d = tempfile.mkdtemp()
    keeper = tool.SnapshotKeeper(d, "GTA5_iter")
    say("\n1. one write (alternating, same trainer, same disk)")
    for rep in range(4):
        torch.cuda.synchronize()
        t = time.time()
        tool.save_atomic(tr.state_dict(), os.path.join(d, "snap.pth"))
        t1 = time.time() - t
        t = time.time()
        ts = tr.training_state()
        t2a = time.time() - t
        t = time.time()
        train_state.save(os.path.join(d, "run.state"), ts, keeper.state(), {"world": 1})
        t2b = time.time() - t
        say(f"  rep {rep}{' (warm-up)' if rep == 0 else ''}: snapshot {t1:.3f} s; train state {t2a + t2b:.3f} s = training_state() {t2a:.3f} + save {t2b:.3f}")
    say(f"  snapshot {os.path.getsize(os.path.join(d, 'snap.pth')) / 1e6:.1f} MB, train state {os.path.getsize(os.path.join(d, 'run.state')) / 1e6:.1f} MB")
    t = time.time()
    ts = train_state.load(os.path.join(d, "run.state"))[0]
    tl = time.time() - t
    t = time.time()
    tr.load_training_state(ts)
    say(f"  train_state.load {tl:.3f} s, load_training_state {time.time() - t:.3f} s")
    del ts

    say(f"\n2. {a.steps} steps on one resident batch, a write every {a.every} steps or none (images/s; warm-up run first, alternating order)")
    on_args = tool.get_arguments(["--train-state", os.path.join(d, "loop.state"), "--train-state-every", str(a.every)])
    off_args = tool.get_arguments([])

    def loop(args):
        flag = tool.TrainStateFile(args, 0, 1, cd)
        torch.cuda.synchronize()
        t0 = time.time()
        for i in range(a.steps):
            tr.step(img, lab)
            flag.after_iteration(i, tr, keeper)
        torch.cuda.synchronize()
        return B * a.steps / (time.time() - t0)
    loop(off_args)
    order = [x for p in range(a.pairs) for x in (("off", "on") if p % 2 == 0 else ("on", "off"))]
    res = {"off": [], "on": []}
    for which in order:
        res[which].append(loop(on_args if which == "on" else off_args))
    say(f"  order {' '.join(order)}")
    for which in ("off", "on"):
        say(f"  {'without writes' if which == 'off' else f'{a.steps // a.every} writes   '}: " + "  ".join(f"{v:.1f}" for v in res[which]) +
            f"   mean {sum(res[which]) / len(res[which]):.1f}")
    del tr
    torch.cuda.empty_cache()

    say(f"\n3. trainV2_simt --synthetic, {a.steps} steps, --train-state-every {a.every} or no --train-state (images/s printed at the last iteration; "
        f"warm-up run first, alternating order)")
    base = ["--synthetic", "--input-size-target", f"{W},{H}", "--batch-size", str(B), "--open-classes", str(K), "--learning-rate", "6e-4",
            "--learning-rate-T", "6e-3", "--num-steps-stop", str(a.steps), "--print-every", str(a.steps - 1), "--save-pred-every", "1000000"]

    def run(which, n):
        flags = ["--train-state", os.path.join(d, f"tool{n}.state"), "--train-state-every", str(a.every)] if which == "on" else []
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            tool.main(base + ["--snapshot-dir", os.path.join(d, f"snap{n}")] + flags)
        lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("iter = ")]
        return float(re.search(r"([0-9.]+) img/s", lines[-1]).group(1))
    run("off", 0)
    res = {"off": [], "on": []}
    for n, which in enumerate(order):
        res[which].append(run(which, n + 1))
    for which in ("off", "on"):
        say(f"  {'without --train-state' if which == 'off' else f'--train-state-every {a.every}'}: " + "  ".join(f"{v:.1f}" for v in res[which]) +
            f"   mean {sum(res[which]) / len(res[which]):.1f}")


if __name__ == "__main__":
    main()
