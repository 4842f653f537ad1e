"""The row-wise kernels, fade-in, conditioning augmentation and WGAN head without a GPU: the float64 restatements of
tests/row_head_cases.py against float64 autograd of the reference's expressions (so that tests/test_row_heads_gpu.py does not hold a
kernel to a copy of itself), and the refusals of the entry points, which happen before any launch."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import row_head_cases as RC  # noqa: E402

RTOL = 1e-12
INVALID, WORKSPACE = -1, -2          # include/t2i_hip.h T2I_ERR_INVALID, T2I_ERR_WORKSPACE (a failed launch is T2I_ERR_LAUNCH = -3)


def close(got, ref):
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(ref, np.float64), rtol=RTOL, atol=0)


# ---- the restatements on their own -----------------------------------------------------------------------------------------
def test_keys_are_the_kernels_keys():
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    assert RC.D_HEAD_KEYS == K.D_HEAD_KEYS and len(K.D_HEAD_KEYS) == 12


@pytest.mark.parametrize('gp_coeff', [10.0, 150.0])
@pytest.mark.parametrize('kt', [None, 0.0, 0.37, 1.0])
@pytest.mark.parametrize('B', [1, 7, 64, 257])
def test_head_restatement_equals_autograd_of_the_reference_loss(B, kt, gp_coeff):
    """oracle/torch_step.py d_step (lines 365-372) on hand-made logits and slopes: the penalty through its own _gp (a [B, 1] gradient
    has the slopes |s|), D_loss / balance_loss / kt_grad by its expressions, the seeds by autograd of D_loss."""
    from oracle import torch_step as T
    ktv = 1.0 if kt is None else float(np.float32(kt))
    for seed in range(4 if B == 1 else 1):
        logits, s1, s2 = (RC.f64(a) for a in RC.head_inputs(B, seed))
        scal, seed_l, seed_s1, seed_s2 = RC.d_head(logits, s1, s2, ktv, gp_coeff)
        l, a, b = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (logits, s1, s2))
        Dg, Dx, Dxmi = l[:B], l[B:2 * B], l[2 * B:]
        real_gp, real_gp2 = T._gp(a.reshape(B, 1)), T._gp(b.reshape(B, 1))
        loss_real, loss_fake, loss_mis = Dx.mean(), Dg.mean(), Dxmi.mean()
        wdist, wdist2 = loss_real - loss_fake, loss_real - loss_mis
        D_loss = -wdist - ktv * wdist2 + gp_coeff * (real_gp + real_gp2)
        gl, ga, gb = torch.autograd.grad(D_loss, [l, a, b])
        wd, wd2 = float(wdist.detach()), float(wdist2.detach())
        ref = dict(D_loss=float(D_loss.detach()), D_loss_real=float(loss_real.detach()), D_loss_fake=float(loss_fake.detach()),
                   D_loss_mismatch=float(loss_mis.detach()), wdist=wd, wdist2=wd2, real_gp=float(real_gp.detach()),
                   real_gp2=float(real_gp2.detach()), reg_loss=float((Dxmi ** 2).mean().detach()), balance_loss=(ktv * wd2 - wd) ** 2,
                   kt_grad=2.0 * (ktv * wd2 - wd) * wd2, kt=ktv)
        assert tuple(scal) == RC.D_HEAD_KEYS
        for k in RC.D_HEAD_KEYS:
            close(scal[k], ref[k])
        close(seed_l, gl.numpy()); close(seed_s1, ga.numpy()); close(seed_s2, gb.numpy())
        # the inputs hold what the GPU cases rely on: a hinge at exactly 1.0 has no seed, and both kinds of hinge occur
        if B >= 3:
            assert s1[RC.HINGE_AT_ONE['s1']] == 1.0 and s2[RC.HINGE_AT_ONE['s2']] == 1.0
            assert seed_s1[0] == 0.0 and seed_s2[-1] == 0.0 and seed_s1[1] == 0.0 and seed_s1[2] > 0.0 and seed_s2[0] > 0.0 and seed_s2[1] == 0.0
            assert scal['real_gp'] != scal['real_gp2'] and scal['real_gp'] > 0.01 and scal['real_gp2'] > 0.01


@pytest.mark.parametrize('which', ['dcode', 'dkl', 'both'])
@pytest.mark.parametrize('n', [1, 1023, 8193])
def test_ca_restatement_equals_autograd(n, which):
    """reference models/wgancls/model.py:117-127: code = mean + exp(log_sigma) * eps, kl = mean(-ls + .5 (-1 + exp(2 ls) + mean^2))"""
    mean, ls, eps = (RC.f64(a) for a in RC.ca_inputs(n))
    rs = np.random.RandomState(n)
    dcode = rs.standard_normal(n) if which != 'dkl' else None
    dkl = 0.7 if which != 'dcode' else None
    m, l = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (mean, ls))
    e = torch.tensor(eps, dtype=torch.float64)
    code_t = m + torch.exp(l) * e
    kl_t = torch.mean(-l + 0.5 * (-1.0 + torch.exp(2.0 * l) + m ** 2))
    out = (code_t * torch.tensor(dcode)).sum() if dcode is not None else 0.0
    out = out + (dkl * kl_t if dkl is not None else 0.0)
    gm, gl = torch.autograd.grad(out, [m, l])
    code, kl = RC.ca_fwd(mean, ls, eps)
    dmean, dls = RC.ca_bwd(mean, ls, eps, dcode, dkl)
    close(code, code_t.detach().numpy()); close(kl, float(kl_t.detach()))
    floor = 1e-15 if dcode is not None else 1e-15 / n       # the two terms of a sum may cancel (and exp(2 ls) - 1 does near ls = 0): a few ulp of a term
    np.testing.assert_allclose(dmean, gm.numpy(), rtol=RTOL, atol=floor)
    np.testing.assert_allclose(dls, gl.numpy(), rtol=RTOL, atol=floor)
    assert float(RC.ca_kl_terms(mean, ls).min()) >= 0.0


def test_the_other_restatements_on_hand_made_values():
    a = np.array([[1.0, -2.0, 3.0, 4.0], [0.5, 0.0, -1.0, 2.0]])
    b = np.array([[2.0, 1.0, 0.0, -1.0], [4.0, 4.0, 4.0, 4.0]])
    s1, s2, a1, a2 = RC.row_moments(a, b)
    close(s1, [6.0, 1.5]); close(s2, [-4.0, 6.0]); close(a1, [10.0, 3.5]); close(a2, [8.0, 14.0])
    close(RC.row_moments(a)[1], [30.0, 5.25])
    close(RC.row_fma2(a, np.array([2.0, -1.0]), b, np.array([0.5, 1.0]), np.array([1.0, 0.0])),
          [[4.0, -2.5, 7.0, 8.5], [3.5, 4.0, 5.0, 2.0]])
    x = np.arange(16.0).reshape(1, 2, 4, 2)
    close(RC.pool2_sum(x, 0.25), np.array([[[[5.0, 6.0], [9.0, 10.0]]]]))
    up = RC.upscale2(x[:, :1, :2], 2.0)
    assert up.shape == (1, 2, 4, 2)
    close(up[0, :, :, 0], [[0.0, 0.0, 4.0, 4.0], [0.0, 0.0, 4.0, 4.0]])
    close((RC.pool2_sum(x, 0.25) * 3.0).sum(), 0.25 * (x * RC.upscale2(np.full((1, 1, 2, 2), 3.0), 1.0)).sum())
    for mode, want in ((0, 0.75 * a + 0.25 * b), (1, 0.25 * a), (2, 0.75 * a)):
        close(RC.lerp(a, b, 0.25, mode), want)
    ss, s = RC.gp_slopes(np.array([[3.0, 4.0], [0.0, 0.0]]))
    close(ss, [25.0, 0.0]); close(s, [5.0, 0.0])
    close(RC.row_scale_div(np.array([[3.0, 4.0], [1.0, 1.0], [2.0, 2.0]]), np.array([10.0, 7.0, 1.0]), np.array([5.0, 0.0, 1e-38])),
          [[6.0, 8.0], [0.0, 0.0], [2.0 / float(np.float32(1e-30))] * 2])
    close(RC.interp(np.array([0.0, 1.0]), a, b), [b[0], a[1]])
    assert len(set(zip(RC.pow2_rows(65, 1), RC.pow2_rows(65, 5), RC.pow2_rows(65, 25)))) == 65
    assert all(u != v for u, v in zip(RC.pow2_rows(65, 1)[:-1], RC.pow2_rows(65, 1)[1:]))


def test_layer_norm_restatement_normalises_each_sample():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 2, 5, 4, generator=g, dtype=torch.float64) * 1.7 + torch.tensor([6.8, -6.8, 0.5], dtype=torch.float64).reshape(3, 1, 1, 1)
    gam, bet = torch.full((4,), 2.0, dtype=torch.float64), torch.full((4,), 0.25, dtype=torch.float64)
    y, dx, dgamma, dbeta = RC.layer_norm(x, gam, bet, torch.ones_like(x))
    xhat = (y - 0.25) / 2.0
    assert float(xhat.mean((1, 2, 3)).abs().max()) < 1e-14
    np.testing.assert_allclose((xhat ** 2).mean((1, 2, 3)).numpy(), 1.0, rtol=1e-10)
    assert float(dx.abs().max()) < 1e-13                       # a constant cotangent with a constant gamma lies in the normaliser's null space
    close(dbeta, [30.0] * 4)


# ---- refusals: every one before any launch, with the entry point named in the message ---------------------------------------
@pytest.fixture(scope='module')
def L():
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    return _lib.lib


def refused(L, name, rc, want=INVALID):
    """On a machine without a GPU a launch fails as well (T2I_ERR_LAUNCH): the code and the message tell a refusal from that."""
    msg = L.t2i_last_error().decode('utf-8', 'replace')
    assert rc == want, (name, rc, msg)
    assert msg.startswith(name + ':'), (name, msg)
    assert ('workspace' in msg) == (want == WORKSPACE), msg


_BUF = (ctypes.c_float * 64)()


@pytest.fixture(scope='module')
def p():
    """a dummy non-null pointer: no refusal reads through it"""
    return ctypes.cast(_BUF, ctypes.c_void_p)


def test_row_moments_workspace_query(L):
    for B in (1, 64, 65):
        assert int(L.t2i_row_moments_workspace_bytes(B)) == B * 64 * 2 * 4
    assert int(L.t2i_row_moments_workspace_bytes(0)) == 0 and int(L.t2i_row_moments_workspace_bytes(-3)) == 0


def test_row_moments_refusals(L, p):
    need = int(L.t2i_row_moments_workspace_bytes(2))
    refused(L, 't2i_row_moments', L.t2i_row_moments(None, None, 2, 8, p, p, p, need, None))
    refused(L, 't2i_row_moments', L.t2i_row_moments(p, None, 0, 8, p, p, p, need, None))
    refused(L, 't2i_row_moments', L.t2i_row_moments(p, None, 2, 0, p, p, p, need, None))
    refused(L, 't2i_row_moments', L.t2i_row_moments(p, None, 2, 8, p, p, p, need - 1, None), WORKSPACE)
    refused(L, 't2i_row_moments', L.t2i_row_moments(p, p, 2, 8, p, p, None, need, None), WORKSPACE)


def test_row_fma2_refusals(L, p):
    refused(L, 't2i_row_fma2', L.t2i_row_fma2(p, p, p, None, None, 2, 8, p, None))          # b without gamma
    refused(L, 't2i_row_fma2', L.t2i_row_fma2(p, None, p, p, None, 2, 8, p, None))          # gamma without b
    refused(L, 't2i_row_fma2', L.t2i_row_fma2(p, None, None, None, None, 2, 8, p, None))    # no alpha


def test_lerp_dev_refusals(L, p):
    refused(L, 't2i_lerp_dev', L.t2i_lerp_dev(p, p, p, -1, 8, p, None))
    refused(L, 't2i_lerp_dev', L.t2i_lerp_dev(p, p, p, 3, 8, p, None))
    refused(L, 't2i_lerp_dev', L.t2i_lerp_dev(p, None, p, 0, 8, p, None))
    refused(L, 't2i_lerp_dev', L.t2i_lerp_dev(p, p, p, 0, 0, p, None))
    refused(L, 't2i_lerp_dev', L.t2i_lerp_dev(p, p, None, 1, 8, p, None))                   # t lives in device memory: no default


@pytest.mark.parametrize('n', [0, (1 << 24) + 1])
def test_ca_kl_refusals(L, p, n):
    refused(L, 't2i_ca_kl_fwd', L.t2i_ca_kl_fwd(p, p, p, n, p, p, None))
    refused(L, 't2i_ca_kl_bwd', L.t2i_ca_kl_bwd(p, p, p, p, p, n, p, p, None))


def test_pool2_sum_refusals(L, p):
    refused(L, 't2i_pool2_sum', L.t2i_pool2_sum(p, 1, 3, 4, 2, 0.25, p, None))               # odd H
    refused(L, 't2i_pool2_sum', L.t2i_pool2_sum(p, 1, 4, 3, 2, 0.25, p, None))               # odd W
    refused(L, 't2i_upscale2', L.t2i_upscale2(p, 1, 2, 2, 0, 1.0, p, None))


def test_wgan_d_head_refusals(L, p):
    args = [p, p, p, p, 4, 150.0, p, p, p, p, None]
    for i in (0, 1, 2, 6, 7, 8, 9):                     # logits, both slope vectors, the three seed outputs, the scalars
        a = list(args)
        a[i] = None
        refused(L, 't2i_wgan_d_head', L.t2i_wgan_d_head(*a))
    a = list(args)
    a[4] = 0
    refused(L, 't2i_wgan_d_head', L.t2i_wgan_d_head(*a))


def test_gp_slopes_refusals(L, p):
    from t2i_amd import _lib
    refused(L, 't2i_gp_slopes', L.t2i_gp_slopes(p, 2, 6, p, _lib.DT_BF16, None))             # bf16 rows need a multiple of 4 elements
    refused(L, 't2i_gp_slopes', L.t2i_gp_slopes(p, 2, 8, p, 7, None))                        # no such dtype
    refused(L, 't2i_row_scale_div', L.t2i_row_scale_div(p, p, None, 2, 8, p, _lib.DT_F32, None))
    refused(L, 't2i_interp', L.t2i_interp(p, p, p, 2, 0, p, None))
