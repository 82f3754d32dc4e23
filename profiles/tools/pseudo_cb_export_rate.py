"""Export rate of make_pseudo_labels over generated full-size frames, one tree and one mode per process (run the parent's tree and this
one alternately):

    python profiles/tools/pseudo_cb_export_rate.py make DIR 16                     # 16 frames of 1024 x 2048 smooth noise + train.txt
    python profiles/tools/pseudo_cb_export_rate.py <tree> confidence|class_balanced DIR

Full-depth DeepLab-v2 (--arch multi, reference_init), fp32, first scale, 8 workers; the export runs once to warm up, then three timed
times (host clock around export(), device synchronised)."""
import json
import os
import sys
import time

if sys.argv[1] == "make":
    import numpy as np
    from PIL import Image
    root, n = sys.argv[2], int(sys.argv[3])
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(root, "train", "city"), exist_ok=True)
    names = []
    for i in range(n):
        small = Image.fromarray(rng.integers(0, 256, (64, 128, 3), dtype=np.uint8))
        img = np.asarray(small.resize((2048, 1024), Image.BICUBIC)).astype(np.int16) + rng.integers(-6, 7, (1024, 2048, 3), dtype=np.int16)
        name = f"city/city_{i:06d}_000019_leftImg8bit.png"
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(root, "train", name))
        names.append(name)
    open(os.path.join(root, "train.txt"), "w").write("".join(x + "\n" for x in names))
    print(sum(os.path.getsize(os.path.join(root, "train", x)) for x in names) / n / 1e6, "MB per frame")
    sys.exit(0)
tree, mode, data = sys.argv[1:4]
sys.path.insert(0, os.path.abspath(tree))
import torch  # noqa: E402
from simt_amd import model_spec as ms  # noqa: E402
from simt_amd.tools import make_pseudo_labels as mpl  # noqa: E402

assert os.path.abspath(mpl.__file__).startswith(os.path.abspath(tree)), mpl.__file__
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
state = ms.reference_init(ms.state_shapes(19, 0, False), seed=3)
lab = mpl.PseudoLabeller(state, num_classes=19, arch="multi", mode=mode, threshold=0.8, device=dev)
kw = dict(portion=0.5, cap=0.9) if mode == "class_balanced" else {}
times = []
for rep in range(4):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    counts = mpl.export(state, data, os.path.join(data, "train.txt"), f"pseudo_{mode}", os.path.join(data, f"pseudo_{mode}.lst"),
                        workers=8, labeller=lab, verbose=False, **kw)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
print("RESULT " + json.dumps({"tree": tree, "mode": mode, "seconds_16_frames": times[1:], "warmup_seconds": times[0],
                              "ignored_share": float(counts[19]) / float(counts.sum())}), flush=True)
