"""The bar of tests/_ntm_ref.py proves itself on the CPU, and the inputs of tests/test_gpu_ntm_solver.py are what they are said to be.

  * Mutants of the fp32 reference, each wrong in one way a kernel of csrc/ntm.hip could be wrong, fail the bar against float64.  For the
    mutants of the W update and of exp_avg_sq the OLD comparison `close(got, ref, 1e-5)` is asked too, and passes them: with the diagonal of
    sig_W at -1e4 it is an absolute 0.1 on W, and exp_avg_sq never exceeds 3e-6 after the first ten steps.
  * The fp32 reference passes its own bar on every input of the GPU tests, with a tau thousands of times below the old bar.
  * The guard input is guarded in fp32 (det = 0, vol = -inf) and not in float64 (det = 1e-205): the GPU expectation is the fp32 decision.
  * The swap input needs row swaps for both NTMs (the float64 Gauss-Jordan mirror counts them) with |det| far above fp32 denormals; on the
    inputs of the main matrix the elimination never swaps.
"""
import math

import numpy as np
import pytest
import torch

import _ntm_ref as nr
from oracle import simt_oracle as so

F32, F64 = torch.float32, torch.float64
INIT = (22, 19, "init", 0, 10, 0, "real")                # the state every older test starts from (golden g4_head_base_k3: Q = 22)
TRAINED = (22, 19, "trained", 10, 10, 0, "real")
_ADAM = so.adam_step_                                    # (inner_ref swaps the module attribute for the mutant while it runs)


def _inner_mutant(c, **kw):
    st, cd, base = nr.inner_case(c)
    base.update(kw)
    return nr.inner_ref(F32, st["ntm"], st["w"], st["m"], st["v"], **base)


def _adam_no_bias_correction(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    m.lerp_(g, 1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    p.addcdiv_(m, v.sqrt().add_(eps), value=-lr)


def _adam_betas_exchanged(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    _ADAM(p, g, m, v, step, lr, beta2, beta1, eps)


def _adam_eps_inside_sqrt(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    m.lerp_(g, 1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    p.addcdiv_(m, (v / (1 - beta2 ** step) + eps).sqrt(), value=-(lr / (1 - beta1 ** step)))


def _adam_v_never_updated(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    keep = v.clone()
    _ADAM(p, g, m, v, step, lr, beta1, beta2, eps)
    v.copy_(keep)


def _adam_w_never_updated(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    keep = p.detach().clone()
    _ADAM(p, g, m, v, step, lr, beta1, beta2, eps)
    p.copy_(keep)


def _adam_narrowed_betas(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """1 - beta and beta^step formed from the betas AFTER narrowing them to fp32 (`1.f - 0.999f` is 1.3e-5 below float(0.001)): what
    ntm_inner_kernel did until this bar was applied to it."""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    m.add_((g - m) * float(np.float32(1) - np.float32(beta1)))
    v.mul_(b2).add_(g * g * float(np.float32(1) - np.float32(beta2)))
    p.addcdiv_(m, (v.sqrt() / math.sqrt(1 - b2 ** step)).add_(eps), value=-(lr / (1 - b1 ** step)))


def _sig_w_diag_not_reset(weight):
    q = weight.shape[0]
    masked = torch.where(torch.eye(q, dtype=torch.bool), torch.full_like(weight, -10000.0), weight)
    return torch.softmax(masked, dim=1) - torch.eye(q, dtype=weight.dtype)


def _hold_inner(got, r64, r32, what, fields=("w", "m", "v", "T", "ntm_grad")):
    for f in fields:
        for k in range(2):
            if r64[f][k] is not None:
                (nr.square_bar if f in ("w", "m", "v") else nr.bar)(got[f][k], r64[f][k], r32[f][k], f"{what} {f}[{k}]")


ADAM_MUTANTS = {"no bias correction": _adam_no_bias_correction, "betas exchanged": _adam_betas_exchanged, "eps inside the root": _adam_eps_inside_sqrt,
                "exp_avg_sq never updated": _adam_v_never_updated, "W never updated": _adam_w_never_updated,
                "1 - beta from the narrowed betas": _adam_narrowed_betas}


@pytest.mark.parametrize("name", sorted(ADAM_MUTANTS))
@pytest.mark.parametrize("case", [INIT, TRAINED], ids=nr.case_id)
def test_adam_mutants_fail_the_bar(case, name):
    r64, r32 = nr.inner_refs(case)
    mut = _inner_mutant(case, adam=ADAM_MUTANTS[name])
    field = {"exp_avg_sq never updated": "v", "1 - beta from the narrowed betas": "v"}.get(name, "w")
    for k in range(2):
        assert nr.rejected(lambda: nr.square_bar(mut[field][k], r64[field][k], r32[field][k], name)), f"{name}: {field}[{k}] passes the bar"
    # why the old assertions go: from the initial state they accept a W that never moved and an exp_avg_sq that is still zero
    if case == INIT and name == "W never updated":
        assert all(nr.old_close_ok(mut["w"][k], r64["w"][k], 1e-5) for k in range(2))
        assert float((mut["w"][0] - r64["w"][0]).abs().max()) > 0.03            # ... although it is off by most of 1 / (Q - 1)
    if case == INIT and name in ("exp_avg_sq never updated", "1 - beta from the narrowed betas"):
        assert all(nr.old_close_ok(mut["v"][k], r64["v"][k], 1e-5) for k in range(2))


def test_step0_ignored_fails_the_bar():
    for case in (TRAINED, (25, 19, "trained", 5000, 10, 1, "real")):
        r64, r32 = nr.inner_refs(case)
        mut = _inner_mutant(case, step0=0)
        assert nr.rejected(lambda: _hold_inner(mut, r64, r32, "step0 ignored", fields=("w",)))


def test_leak_mutants_fail_the_bar():
    for case in (INIT, TRAINED):
        st, _, _ = nr.inner_case(case)
        r64, r32 = nr.inner_refs(case)
        dropped = dict(r32, ntm_grad=[g.clone() for g in st["ntm_grad"]])
        assigned = dict(r32, ntm_grad=[r32["ntm_grad"][k] - st["ntm_grad"][k] for k in range(2)])
        for what, mut in (("leak dropped", dropped), ("leak assigned, not accumulated", assigned)):
            assert nr.rejected(lambda: _hold_inner(mut, r64, r32, what, fields=("ntm_grad",))), what
            _hold_inner(mut, r64, r32, what, fields=("w", "m", "v", "T"))          # (nothing else moved)


def test_diagonal_not_reset_fails():
    r64, r32 = nr.inner_refs(TRAINED)
    mut = _inner_mutant(TRAINED, sig_w=_sig_w_diag_not_reset)
    assert nr.rejected(lambda: _hold_inner(mut, r64, r32, "diagonal not reset", fields=("w",)))
    off = nr.offdiag(22)
    assert torch.equal(mut["w"][0][off], r32["w"][0][off])                          # ... and the diagonal is all that differs


def test_post_mutants_fail_the_bar():
    # the anchor term over all rows instead of the `ex` rows
    c = (22, 19, "trained", "mixed", "train", 0, "real")
    st, cd, hout, kw = nr.post_case(c)
    r64, r32 = nr.post_refs(c)
    mut = nr.post_ref(F32, st["ntm"], st["w"], hout, mutant="anchor_all_rows", **kw)
    for k in range(2):
        assert nr.rejected(lambda: nr.bar(mut["ntm_grad"][k], r64["ntm_grad"][k], r32["ntm_grad"][k], "anchor over all rows"))
    assert nr.rejected(lambda: nr.scalars_close(mut["lout"], r64["lout"], [8], "anchor over all rows"))
    # the volume gradient applied although the guard fired: NaN for the degenerate NTM, a finite but wrong gradient for the healthy one
    for name in ("guard_both", "guard_one"):
        ntm, w, cd, hout, kw, _ = nr.special_post_case(name)
        r64, r32 = nr.special_post_refs(name)
        mut = nr.post_ref(F32, ntm, w, hout, mutant="vol_while_guarded", **kw)
        assert mut["guarded"]
        for k in range(2):
            assert nr.rejected(lambda: nr.bar(mut["ntm_grad"][k], r64["ntm_grad"][k], r32["ntm_grad"][k], "volume gradient while guarded")), (name, k)
        assert not bool(torch.isfinite(mut["ntm_grad"][0]).all()) and (name == "guard_both" or bool(torch.isfinite(mut["ntm_grad"][1]).all()))


def test_every_gpu_input_the_fp32_reference_passes_its_own_bar():
    """... and the bar is tight: no tau above 1e-4.  (The old bar on W: 1e-5 * (1 + 1e4) = 0.1 absolute against entries of 0.05.)"""
    taus = []
    for c in nr.INNER_CASES:
        r64, r32 = nr.inner_refs(c)
        for f in ("w", "m", "v", "T", "ntm_grad"):
            for k in range(2):
                if r64[f][k] is not None:
                    r = (nr.square_bar if f in ("w", "m", "v") else nr.bar)(r32[f][k], r64[f][k], r32[f][k], f"{nr.case_id(c)} {f}[{k}]")
                    nr.report(nr.case_id(c), f"{f}[{k}] fp32 reference", r)
                    taus.append(r["tau"])
    for c in list(nr.POST_CASES) + ["swap", "guard_both", "guard_one"]:
        r64, r32 = nr.special_post_refs(c) if isinstance(c, str) else nr.post_refs(c)
        tag = c if isinstance(c, str) else nr.case_id(c)
        for k in range(2):
            if r64["ntm_grad"][k] is not None:
                r = nr.bar(r32["ntm_grad"][k], r64["ntm_grad"][k], r32["ntm_grad"][k], f"{tag} ntm_grad[{k}]")
                nr.report(tag, f"ntm_grad[{k}] fp32 reference", r)
                taus.append(r["tau"])
        if not r64["guarded"]:
            nr.scalars_close(r32["lout"], r64["lout"], range(13), tag)
    assert max(taus) <= 1e-4, max(taus)


def test_guard_input_is_guarded_in_fp32_only():
    for name in ("guard_both", "guard_one"):
        ntm, w, cd, hout, kw, _ = nr.special_post_case(name)
        r32 = nr.post_ref(F32, ntm, w, hout, **kw)
        free64 = nr.post_ref(F64, ntm, w, hout, **kw)
        assert r32["guarded"] and float(r32["vol"][0]) == -math.inf                     # det(T1^T T1) == 0 in fp32
        assert not free64["guarded"] and -240.0 < float(free64["vol"][0]) < -230.0       # 0.5 log 1.2e-205 in float64
        assert math.isfinite(float(r32["vol"][1])) == (name == "guard_one")
        assert float(r32["lout"][7]) == 0.0 and float(r32["lout"][9]) == 0.0
        assert all(bool(torch.isfinite(g).all()) for g in r32["ntm_grad"])


def test_swap_input_needs_a_swap_and_the_main_matrix_none():
    cd, ntm = nr.swap_input()
    counts = []
    for n in ntm:
        det, inv, swaps = nr.swaps_of(n, cd, 19)
        T = so.sig_ntm_forward(n.double(), cd.double(), 19)
        G = (T.t() @ T).numpy()
        assert swaps >= 1 and abs(det) > 1e-30
        np.testing.assert_allclose(det, np.linalg.det(G), rtol=1e-9)                   # the mirror is a determinant ...
        np.testing.assert_allclose(inv @ G, np.eye(19), atol=1e-9)                       # ... and an inverse
        counts.append(swaps)
    # `det` without the swap sign folded into |.|: an odd number of swaps makes the product of the pivots negative, log sqrt of it NaN, and the
    # guard would fire on a healthy matrix -- the scalar checks of the GPU test see that
    assert any(s % 2 == 1 for s in counts)
    r64, r32 = nr.special_post_refs("swap")
    assert not r64["guarded"] and not r32["guarded"]
    mut = r64["lout"].clone()
    for k, s in enumerate(counts):
        mut[10 + k] = torch.log(torch.sqrt(torch.exp(2 * r64["lout"][10 + k]) * (-1.0) ** s))
    mut[7] = mut[10] + mut[11]
    assert nr.rejected(lambda: nr.scalars_close(mut, r64["lout"], [7, 10, 11], "no swap sign"))
    for c in nr.POST_CASES:
        st, cd, _, _ = nr.post_case(c)
        for k in ((1,) if c[5] else (0, 1)):
            assert nr.swaps_of(st["ntm"][k], cd, c[1])[2] == 0, (c, k)
