"""The label launches of csrc/label_sweep.hip against a RECORDING: tests/golden/g17_label_sweep.npz holds what the library of the commit before
the sweep (one __global__ function per launch, csrc/eval_metric.hip) wrote for the cases of tests/_label_sweep_cases.py, and the shipped
library must reproduce every array byte for byte.

The other tests of these launches hold them to one another (online labels to the export, the export's mode 0 to the evaluator, the
class-balanced launches to compositions of confidence-mode launches); since the launches share one kernel body those equalities hold by
construction, and only a recording made outside that body can tell a change of the arithmetic.  By construction this test passed at the
commit that was recorded: what it covers is equality with a fixed recording, which no other test does.

Cases: the eight geometries and five thresholds of tests/test_gpu_online_labels.py (both families, W % 4 != 0, a pixel count that is no
multiple of the block, the scalar-gather path, NaN pixels, exact ties) through every entry point that accepts the family; P = 3 (the
byte-store tail); P = 525 825, just above block x grid cap of both launch shapes (a second grid-stride trip), maps held as SHA-256.
The fixture also holds the SHA-256 of every generated input: a generator that drifts (numpy) is reported as that, not as a kernel failure.
"""
import json

import numpy as np
import pytest

import _label_sweep_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(K.GOLDEN) as z:
        return json.loads(str(z["index"])), {k: z[k] for k in z.files if k.startswith("blob_")}


def test_cases_are_the_online_label_tests_geometries():
    import test_gpu_online_labels as OL
    assert K.GEOMETRIES == OL.GEOMETRIES and [repr(t) for t in K.THRESHOLDS] == [repr(t) for t in OL.THRESHOLDS]


@pytest.mark.parametrize("name", list(K.CASES))
def test_library_reproduces_the_recording_byte_for_byte(dev, golden, name):
    index, blobs = golden
    drift = [k for k, v in K.input_digests(name).items() if index["inputs"][name][k] != v]
    assert not drift, f"the input generator drifted ({drift}): re-record the fixture from commit {index['parent_commit']}, the kernels were not run"
    got = K.run(name, dev)
    want = {k[len(name) + 1:]: blobs["blob_" + sha] for k, sha in index["outputs"].items() if k.startswith(name + "/")}
    assert sorted(got) == sorted(want), "the case table and the fixture differ"
    bad = []
    for key, arr in got.items():
        a, w = K.stored(name, key, arr), want[key]
        if a.dtype != w.dtype or a.shape != w.shape or a.tobytes() != w.tobytes():
            bad.append(key if a.shape != arr.shape or a.shape != w.shape else f"{key} ({int((a != w).sum())} of {a.size} elements)")
    assert not bad, f"{len(bad)} of {len(got)} outputs differ from the recording of {index['parent_commit'][:12]}: {bad[:12]}"
    maps = [k for k, arr in got.items() if K.is_map(name, arr)]
    assert len(maps) >= 30
