"""The differentiable augmentation T of DESIGN.md section 4.35 restated in plain torch (any dtype; the tests use float64 and let autograd
differentiate it), and the hand-made parameter rows of tests/test_diffaug_gpu.py and tests/test_pggan_diffaug_gpu.py.

A row is (b, s, c, ty, tx, y0, y1, x0, x1).  The restatement follows the definition literally, one step per line, with a Python loop
over the samples for the shift; like the kernels it does not read the columns of a policy that is not named."""
import numpy as np
import torch

POLICIES = ('color', 'translation', 'cutout', 'color,translation,cutout')
ALL = POLICIES[-1]

# shape -> rows.  Shifts within r = int(size / 8 + 0.5), rectangles of the publication's extent int(size / 2 + 0.5) unless a border clips them.
ROWS = {
    (2, 4, 4, 3): [(0.2, 0.5, 1.3, 1, -1, 1, 3, 0, 2),                    # stage 1: shift 1, cut 2
                   (-0.3, 1.6, 0.7, -1, 0, 0, 2, 2, 4)],
    (3, 5, 7, 3): [(0.1, 0.3, 0.8, 1, 1, 1, 4, 2, 6),                     # odd, non-square; extents 3 (odd) and 4
                   (-0.4, 1.9, 1.4, -1, 0, 0, 2, 0, 3),                   # clipped at the top and the left
                   (0.45, 1.0, 0.5, 0, -1, 3, 5, 4, 7)],                  # clipped at the bottom and the right
    (2, 8, 8, 4): [(0.25, 0.1, 1.2, -1, 1, 2, 6, 3, 7),                   # C = 4
                   (-0.15, 1.7, 0.6, 1, 0, 5, 8, 0, 2)],
    (4, 16, 16, 3): [(0.3, 0.4, 1.45, 2, -2, 0, 4, 4, 12),                # r = 2: ty = +r, tx = -r; rectangle clipped at the top
                     (-0.5, 2.0, 0.5, -2, 2, 12, 16, 2, 10),              # the reverse; clipped at the bottom
                     (0.05, 1.2, 0.9, 2, 2, 3, 11, 0, 4),                 # clipped at the left
                     (-0.2, 0.0, 1.1, -2, -2, 5, 13, 12, 16)],            # clipped at the right; s = 0
    (2, 64, 64, 3): [(0.35, 0.6, 1.25, 8, -5, 10, 42, 20, 52),            # more than one partial sum per sample
                     (-0.45, 1.5, 0.75, -3, 8, 40, 64, 0, 17)],
    (1, 256, 256, 3): [(0.15, 1.3, 0.65, -32, 21, 100, 228, 0, 90)],      # the largest stage
}
SHAPES = list(ROWS)


def table(shape, dtype=torch.float32):
    return torch.tensor(ROWS[tuple(shape)], dtype=dtype)


def identity_table(n, dtype=torch.float32):
    return torch.tensor([(0.0, 1.0, 1.0, 0, 0, 0, 0, 0, 0)] * n, dtype=dtype)


def drawn_table(n, H, W, seed):
    """[n, 9] float64 from the publication's distributions through numpy's RandomState (a stream that does not change between
    versions): the tables of the model-level tests."""
    rs = np.random.RandomState(seed)
    P = np.zeros((n, 9))
    P[:, 0], P[:, 1], P[:, 2] = rs.uniform(-0.5, 0.5, n), rs.uniform(0.0, 2.0, n), rs.uniform(0.5, 1.5, n)
    for col, size in ((3, H), (4, W)):
        r = int(size / 8.0 + 0.5)
        P[:, col] = rs.randint(-r, r + 1, n)
    for col, size in ((5, H), (7, W)):
        ext = int(size / 2.0 + 0.5)
        lo = rs.randint(0, size - ext % 2 + 1, n) - ext // 2
        P[:, col], P[:, col + 1] = np.maximum(lo, 0), np.minimum(lo + ext, size)
    return torch.tensor(P, dtype=torch.float64)


def ref_T(x, P, policy=ALL, offset=True):
    """T(x) for x [B,H,W,C] and P [B,9] of x's dtype, by the definition; differentiable by autograd to any order."""
    names = policy.split(',')
    B, H, W, C = x.shape
    col = lambda j: P[:, j].reshape(B, 1, 1, 1).to(x.dtype)
    u = x
    if 'color' in names:
        b, s, c = col(0), col(1), col(2)
        if offset:
            u = u + b
        u = s * u + (1 - s) * u.mean(3, keepdim=True)
        u = c * u + (1 - c) * u.mean((1, 2, 3), keepdim=True)
    if 'translation' in names:
        out = torch.zeros_like(u)
        for n in range(B):
            ty, tx = int(P[n, 3]), int(P[n, 4])
            ya, yb, xa, xb = max(ty, 0), min(H + ty, H), max(tx, 0), min(W + tx, W)        # destination rows / columns
            if ya < yb and xa < xb:
                out[n, ya:yb, xa:xb] = u[n, ya - ty:yb - ty, xa - tx:xb - tx]
        u = out
    if 'cutout' in names:
        mask = torch.ones(B, H, W, 1, dtype=x.dtype)
        for n in range(B):
            y0, y1, x0, x1 = (int(P[n, j]) for j in (5, 6, 7, 8))
            mask[n, y0:y1, x0:x1] = 0
        u = u * mask.to(u.device)
    return u


def second_order(T, x, w):
    """The chain of the gradient penalty on T alone: y = T(x), gx = d sum(w y^2) / dx with its graph, loss = sum(gx^2)
    -> (y, gx, d loss / dx, d loss / dw), detached."""
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    y = T(x)
    gx, = torch.autograd.grad((w * y * y).sum(), x, create_graph=True)
    dx, dw = torch.autograd.grad((gx * gx).sum(), [x, w])
    return y.detach(), gx.detach(), dx.detach(), dw.detach()


def inputs(shape, seed=0):
    """x ~ N(0, 1) and w ~ U(0.5, 1.5), float32, from numpy's RandomState"""
    rs = np.random.RandomState(1000 + seed + sum(shape))
    return torch.tensor(rs.standard_normal(shape), dtype=torch.float32), torch.tensor(rs.uniform(0.5, 1.5, shape), dtype=torch.float32)


def relerr(got, ref):
    """max-norm relative error"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))
