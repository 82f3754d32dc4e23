"""Per-frame class statistics of the labelled source set, for rare-class sampling (simt_amd/data/rare_class.py, --rcs-stats).

  python -m simt_amd.tools.compute_class_stats --data-dir D --data-list L --out FILE [--num-classes 19] [--num-workers N]

Reads every label of GTA5DataSet(D, L) through `decode()` -- the GTA5 ids are train ids by then -- and writes JSON:
  {"n_classes": C, "ignore_label": 255, "list_sha256": ..., "items": [{"name": ..., "counts": [C ints]}, ...]}
counts = np.bincount of the FULL-SIZE label; 255 and every label >= C are not counted.  Host only: no GPU, no library.  The file is written
to a temporary name and renamed, so a reader never sees a partial one.
"""
import argparse
import hashlib
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

IGNORE_LABEL = 255


def label_counts(lab, n_classes):
    """uint8 labels of any shape -> int64 [n_classes]: the pixels of every class below n_classes."""
    return np.bincount(np.asarray(lab, dtype=np.uint8).reshape(-1), minlength=256)[:n_classes].astype(np.int64)


def compute(dataset, n_classes, num_workers=4):
    """-> the list of {"name", "counts"} records of `dataset`, in list order."""
    def one(i):
        _rgb, lab, name = dataset.decode(i)
        return {"name": name, "counts": label_counts(lab, n_classes).tolist()}
    with ThreadPoolExecutor(max(1, int(num_workers))) as pool:
        return list(pool.map(one, range(len(dataset))))


def save_json_atomic(obj, path):
    tmp = f"{path}.{os.getpid()}.tmp"
    try:
        with open(tmp, "w") as f:
            json.dump(obj, f)
            f.write("\n")
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def main(argv=None):
    p = argparse.ArgumentParser(description="per-frame class pixel counts of a GTA5 list, for --rare-class-sampling")
    p.add_argument("--data-dir", required=True)
    p.add_argument("--data-list", required=True)
    p.add_argument("--out", required=True)
    p.add_argument("--num-classes", type=int, default=19)
    p.add_argument("--num-workers", type=int, default=4)
    args = p.parse_args(argv)
    if not 1 <= args.num_classes <= IGNORE_LABEL:
        raise SystemExit(f"--num-classes {args.num_classes}: 1 to {IGNORE_LABEL}")
    from simt_amd.dataset.gta5_dataset import GTA5DataSet
    ds = GTA5DataSet(args.data_dir, args.data_list, ignore_label=IGNORE_LABEL)
    with open(args.data_list, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    items = compute(ds, args.num_classes, args.num_workers)
    save_json_atomic({"n_classes": args.num_classes, "ignore_label": IGNORE_LABEL, "list_sha256": sha, "items": items}, args.out)
    total = np.sum([it["counts"] for it in items], axis=0)
    print(f"{args.out}: {len(items)} frames, {int(total.sum())} counted pixels, frames per class "
          f"{[int(sum(1 for it in items if it['counts'][c] > 0)) for c in range(args.num_classes)]}")


if __name__ == "__main__":
    main()
