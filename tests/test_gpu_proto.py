"""simt_proto_rectify / simt_proto_accumulate / simt_proto_update on the GPU (csrc/proto.hip) against the float64 restatement of
tests/_proto_ref.py fed the same stored inputs.  The value bar is  max|gpu - f64| <= 4 * err32 + 2^-22 * max|f64|,  err32 the error of the
sequential float32 restatement -- never the kernels' own figure; the discrete outputs are exact outside the exclusion set, whose share the
inputs keep below 1 % (tests/test_proto_cpu.py asserts that for the float32 restatement alone).  Measured gpu_err / err32 per case:
profiles/proto_denoise.txt.  Row offsets are 64-bit in all three kernels (m * ldF with m < 2^31): no size here reaches an index past 2^31,
which would take a 16 GB feature map."""
import ctypes as C

import numpy as np
import pytest
import torch

import _proto_ref as pr
from simt_amd import _lib as L
from simt_amd import ops

pytestmark = pytest.mark.gpu
GUARD = 64          # elements in front of and behind every output
NAN_WORD = 0x7FC00001          # a NaN pattern no launch produces


class _Step:
    """The buffers and descriptors of the three launches over a case of _proto_ref.make_case; run() -> the dict check_step takes."""

    def __init__(self, dev, k):
        self.k, self.dev = k, dev
        self.M, self.D, self.Cn, self.ldp, self.ldF = k["M"], k["D"], k["C"], k["ldp"], k["ldF"]
        self.dtype = torch.bfloat16 if k["bf16"] else torch.float32
        self.F = torch.from_numpy(k["F"]).to(dev).to(self.dtype).contiguous()
        assert np.array_equal(self.F.float().cpu().numpy(), k["F"], equal_nan=True), "the device holds other feature values than the restatement reads"
        self.P = torch.from_numpy(k["P"]).to(dev).contiguous()
        lib = L.load()
        self.parts, self.words = lib.simt_proto_parts(self.M), lib.simt_proto_ws_floats(self.M, self.Cn, self.D)
        self.aparts = -(-self.M // pr.PART_CELLS)
        assert self.parts == min(-(-self.M // 8), 2048) and self.words == self.aparts * self.Cn * (self.D + 1)
        n = dict(out=self.M * self.ldp, lab=self.M, changed=self.parts, ws=self.words, eta=self.Cn * self.D, n=self.Cn)
        kinds = dict(out=torch.float32, lab=torch.uint8, changed=torch.int32, ws=torch.float32, eta=torch.float32, n=torch.int32)
        self.size = n
        self.buf = {q: torch.empty(n[q] + 2 * GUARD, device=dev, dtype=kinds[q]) for q in n}
        self.desc = self.make()

    def view(self, q):
        return self.buf[q][GUARD:GUARD + self.size[q]]

    def make(self, **kw):
        k, v = self.k, self.view
        r, a, u = L.ProtoRectifyDesc(), L.ProtoAccDesc(), L.ProtoUpdateDesc()
        r.F, r.P, r.out, r.eta, r.n = self.F.data_ptr(), self.P.data_ptr(), v("out").data_ptr(), v("eta").data_ptr(), v("n").data_ptr()
        r.lab, r.changed_part = v("lab").data_ptr(), v("changed").data_ptr()
        r.M, r.D, r.ldF, r.C, r.ldp, r.dtype, r.family, r.temp, r.thr = self.M, self.D, self.ldF, self.Cn, self.ldp, ops.dt_code(self.dtype), \
            k["family"], k["temp"], k["thr"]
        a.F, a.lab, a.ws, a.M, a.D, a.ldF, a.C, a.dtype = self.F.data_ptr(), v("lab").data_ptr(), v("ws").data_ptr(), self.M, self.D, self.ldF, \
            self.Cn, ops.dt_code(self.dtype)
        u.ws, u.eta, u.n, u.M, u.D, u.C, u.momentum = v("ws").data_ptr(), v("eta").data_ptr(), v("n").data_ptr(), self.M, self.D, self.Cn, k["momentum"]
        for key, val in kw.items():
            which, field = key.split("__")
            setattr(dict(r=r, a=a, u=u)[which], field, val)
        return r, a, u

    def poison(self, eta=None, n=None):
        for q, t in self.buf.items():
            if t.dtype == torch.float32:
                t.view(torch.int32).fill_(NAN_WORD)
            else:
                t.fill_(0x5A if t.dtype == torch.uint8 else -7)
        self.view("eta").copy_(torch.from_numpy(np.ascontiguousarray(self.k["eta"] if eta is None else eta, dtype=np.float32).reshape(-1)))
        self.view("n").copy_(torch.from_numpy(np.ascontiguousarray(self.k["n"] if n is None else n, dtype=np.int32)))

    def guards_intact(self):
        for q, t in self.buf.items():
            for g in (t[:GUARD], t[GUARD + self.size[q]:]):
                want = NAN_WORD if t.dtype == torch.float32 else 0x5A if t.dtype == torch.uint8 else -7
                assert bool(((g.view(torch.int32) if t.dtype == torch.float32 else g) == want).all()), f"{q}: a guard word was written"

    def run(self, desc=None, launches=3, **state):
        self.poison(**state)
        r, a, u = desc or self.desc
        st = ops.stream_ptr()
        L.call("simt_proto_rectify", C.byref(r), st)
        if launches > 1:
            L.call("simt_proto_accumulate", C.byref(a), st)
        if launches > 2:
            L.call("simt_proto_update", C.byref(u), st)
        torch.cuda.synchronize()
        self.guards_intact()
        got = dict(out=self.view("out").view(self.M, self.ldp).cpu().numpy(), lab=self.view("lab").cpu().numpy(),
                   changed_part=self.view("changed").cpu().numpy(), eta=self.view("eta").view(self.Cn, self.D).cpu().numpy(),
                   n=self.view("n").cpu().numpy(), ws=self.view("ws").cpu().numpy())
        got["changed"] = int(got["changed_part"].sum())
        if launches > 1:
            sums = got["ws"][:self.aparts * self.Cn * self.D].reshape(self.aparts, self.Cn, self.D)
            S = np.zeros((self.Cn, self.D), dtype=np.float32)
            for p in range(self.aparts):          # part order, as simt_proto_update adds them
                S = (S + sums[p]).astype(np.float32)
            got["S"] = S
            got["cnt"] = got["ws"][self.aparts * self.Cn * self.D:].view(np.int32).reshape(self.aparts, self.Cn).sum(axis=0)
        return got


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, keys=("out", "lab", "changed_part", "ws", "eta", "n")):
    for q in keys:
        assert np.array_equal(_words(a[q]), _words(b[q])), f"{q}: the words differ"


@pytest.mark.parametrize("name", list(pr.CASES))
def test_step_vs_float64(dev, name):
    k = pr.case(name)
    run = _Step(dev, k)
    got = run.run()
    pr.check_step(got, k, report=name)
    assert int(got["changed"]) > 0 or k["M"] <= 9
    _same(got, run.run())          # a second run of the three launches repeats the first word for word


@pytest.mark.parametrize("family", [0, 1])
def test_no_class_seen_is_a_copy_and_the_first_update_is_the_mean(dev, family):
    k = dict(pr.make_case(2 * 7 * 9, 256, 19, bf16=True, family=family, ldp=24, seed=21), thr=float("-inf"))
    run = _Step(dev, k)
    junk = np.full((19, 256), np.nan, dtype=np.float32)
    got = run.run(eta=junk, n=np.zeros(19, np.int32))
    assert np.array_equal(_words(got["out"]), _words(k["P"])), "no class seen: out is not P word for word"
    assert got["changed"] == 0 and np.array_equal(got["lab"], pr.first_argmax(k["P"][:, :19]).astype(np.uint8))
    S, cnt = pr.accumulate_ref(pr.features(k), got["lab"], 19, np.float64)
    assert np.array_equal(got["cnt"], cnt) and np.array_equal(got["n"], (cnt > 0).astype(np.int32))
    live = cnt > 0
    assert live.sum() >= 10 and np.isfinite(got["eta"][live]).all()
    mean = S[live] / cnt[live][:, None]
    s32, _ = pr.accumulate_ref(pr.features(k), got["lab"], 19, np.float32)
    err32 = np.abs((s32[live] / cnt[live][:, None].astype(np.float32)).astype(np.float64) - mean).max()
    assert np.abs(got["eta"][live] - mean).max() <= pr.FACTOR * err32 + pr.REL * np.abs(mean).max()
    assert np.array_equal(_words(got["eta"][~live]), _words(junk[~live])), "a class absent from the batch moved"


@pytest.mark.parametrize("family", [0, 1])
def test_an_unseen_class_is_never_read_and_not_penalised(dev, family):
    k = pr.make_case(2 * 6 * 6, 512, 19, family=family, ldp=20, unseen=3, seed=22)
    gone = np.nonzero(k["n"] == 0)[0]
    assert len(gone) == 3
    run = _Step(dev, k)
    a = run.run(launches=1)
    for fill in (0.0, 1.0e30, float("inf")):
        eta = k["eta"].copy()
        eta[gone] = fill
        _same(a, run.run(launches=1, eta=eta), keys=("out", "lab", "changed_part"))
    if family == 1:          # z = -0: the logit of an unseen class is the teacher's, word for word
        assert np.array_equal(_words(a["out"][:, gone]), _words(k["P"][:, gone]))
    pr.check_step(run.run(), k)


def test_nan_and_inf_rows_poison_their_own_cell_and_class(dev):
    k = dict(pr.make_case(3 * 7 * 7, 2048, 19, bf16=True, seed=23), thr=float("-inf"))
    clean = _Step(dev, k).run()
    F = k["F"].copy()
    F[3, 5], F[10, 0], F[11, :] = np.nan, np.inf, -np.inf
    hit = [3, 10, 11]
    got = _Step(dev, dict(k, F=F)).run()
    assert (got["lab"][hit] == 255).all() and np.isnan(got["out"][hit, :19]).all()
    rest = np.setdiff1d(np.arange(k["M"]), hit)
    assert np.array_equal(_words(got["out"][rest]), _words(clean["out"][rest])) and np.array_equal(got["lab"][rest], clean["lab"][rest])
    lost = np.unique(clean["lab"][hit])          # the classes those cells would have fed: their sums lose a cell, nobody else's moves
    others = np.setdiff1d(np.arange(19), lost)
    assert np.array_equal(_words(got["eta"][others]), _words(clean["eta"][others])) and np.array_equal(got["n"], clean["n"])
    assert np.isfinite(got["S"]).all() and int(got["cnt"].sum()) == int(clean["cnt"].sum()) - 3
    k2 = dict(k, F=F)
    pr.check_step(got, k2)


def test_refusals_write_nothing(dev):
    k = pr.case("f32_2x8x16_256_25_logits")
    run = _Step(dev, k)
    run.poison()
    before = {q: t.clone() for q, t in run.buf.items()}
    m = run.make
    bad_r = [m(**{"r__" + f: None}) for f in ("F", "P", "out", "eta", "n", "lab", "changed_part")]
    bad_r += [m(r__M=0), m(r__M=1 << 31), m(r__C=1), m(r__C=65), m(r__D=0), m(r__D=252), m(r__D=4104), m(r__ldF=248), m(r__ldF=260), m(r__ldp=24),
              m(r__dtype=2), m(r__dtype=-1), m(r__family=2), m(r__temp=0.0), m(r__temp=-1.0), m(r__temp=float("nan")), m(r__temp=float("inf")),
              m(r__thr=float("nan")), m(r__F=run.F.data_ptr() + 8), m(r__eta=run.view("eta").data_ptr() + 4), m(r__P=run.P.data_ptr() + 2),
              m(r__out=run.view("out").data_ptr() + 2)]
    bad_a = [m(**{"a__" + f: None}) for f in ("F", "lab", "ws")]
    bad_a += [m(a__M=0), m(a__M=1 << 31), m(a__C=1), m(a__C=65), m(a__D=4), m(a__D=4104), m(a__ldF=248), m(a__ldF=260), m(a__dtype=3),
              m(a__F=run.F.data_ptr() + 8), m(a__ws=run.view("ws").data_ptr() + 4)]
    bad_u = [m(**{"u__" + f: None}) for f in ("ws", "eta", "n")]
    bad_u += [m(u__M=0), m(u__C=65), m(u__C=0), m(u__D=12), m(u__momentum=1.0), m(u__momentum=-0.1), m(u__momentum=float("nan")),
              m(u__ws=run.view("ws").data_ptr() + 4), m(u__eta=run.view("eta").data_ptr() + 8)]
    st = ops.stream_ptr()
    for name, i, descs in (("simt_proto_rectify", 0, bad_r), ("simt_proto_accumulate", 1, bad_a), ("simt_proto_update", 2, bad_u)):
        for d in descs:
            with pytest.raises(L.SimtHipError):
                L.call(name, C.byref(d[i]), st)
        with pytest.raises(L.SimtHipError):
            L.call(name, None, st)
    torch.cuda.synchronize()
    for q, t in run.buf.items():
        same = torch.equal(t.view(torch.int32), before[q].view(torch.int32)) if t.dtype == torch.float32 else torch.equal(t, before[q])
        assert same, f"{q}: a refused launch wrote"
    lib = L.load()
    assert lib.simt_proto_parts(0) == 0 and lib.simt_proto_parts(1 << 31) == 0 and lib.simt_proto_parts(17) == 3
    assert lib.simt_proto_ws_floats(0, 19, 2048) == 0 and lib.simt_proto_ws_floats(100, 65, 2048) == 0 and lib.simt_proto_ws_floats(100, 19, 12) == 0
    assert lib.simt_proto_ws_floats(37636, 19, 2048) == 148 * 19 * 2049
