"""Closed forms of the two Lovasz losses with every option of the reference (per_image, ignore, only_present), written for this project
from the semantics DESIGN.md section 26 pins: float64 by default, float32 (`dtype`) as the yardstick of the fp32 operation sequence,
and the same losses as differentiable torch expressions for the autograd cross-check.  Also the exactly representable cases the GPU
tests sort.

Conventions: the hinge takes z, t [B,P]; the softmax form p, t [B,C,HW] with the void value in EVERY target plane of a void pixel.
Ties keep ascending flat index (torch.sort(stable=True)); void elements are removed before the sort, as the reference compacts them.

Importable without a GPU and without the built library."""
import zlib

import torch
import torch.nn.functional as F

F64 = torch.float64
VOID = 255.0

# (N, B, P or HW) of the operator-level GPU tests: the sizes at which the form of the sort changes (one workgroup below 4096, the split
# form up to 131072, the long-row form above) and rows whose last segment holds one or two elements
FLAT_SIZES = [(1, 1, 1), (2, 2, 1), (255, 3, 85), (4095, 1, 4095), (4096, 2, 2048), (4098, 3, 1366), (131072, 2, 65536),
              (131073, 1, 131073), (133121, 1, 133121), (133122, 3, 44374)]
SOFTMAX_C = 2
# Share of positive labels in the cases.  g_k = J_k - J_(k-1) in fp32 is off by up to 2^-23 whatever the row length (each J_k carries one
# correctly rounded division of a value just below 1), while the largest gradient of a row with G positives is 1 / G; so the gradient bar
# 5e-3 max|ref| can only hold while 2^-23 G <= 5e-3, G <= 41 943.  One positive in 8 keeps G near 16 700 in the longest row (133 122);
# the reference's own fp32 sequence, which the kernels reproduce bit for bit, cannot meet the bar on rows with more positives than that
# (measured with one in 2: 5.8e-3 at G = 65 500, by the one-workgroup kernel and the split form as much as by the long-row form).
POSITIVE_ONE_IN = 8


def gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def jaccard_gradient(fg_sorted, dtype=F64):
    """g_k = J_k - J_(k-1), J_k = 1 - (G - c_k) / (G + k - c_k), in `dtype` with the reference's operation sequence"""
    fg = fg_sorted.to(dtype)
    G = fg.sum()
    jac = 1.0 - (G - fg.cumsum(0)) / (G + (1.0 - fg).cumsum(0))
    if fg.numel() > 1:
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
    return jac


def _errors(x, lab, kind):
    """(sorted quantity, what enters the dot product, d value / d x) of the valid elements"""
    if kind == 'hinge':
        s = 2.0 * lab - 1.0
        e = 1.0 - x * s
        return e, F.elu(e), -s * torch.where(e > 0, torch.ones_like(e), torch.exp(e))
    e = (lab - x).abs()
    d = torch.where(lab > 0.5, -torch.ones_like(e), torch.ones_like(e))
    return e, e, torch.where(e == 0, torch.zeros_like(e), d)                    # torch's abs backward is 0 at 0


def row(x, t, ignore, kind, dtype=F64):
    """one row: x, t 1-D -> (loss, d loss / d x with zeros at the void elements, positives among the valid elements)"""
    valid = torch.ones_like(t, dtype=torch.bool) if ignore is None else (t != ignore)
    grad = torch.zeros(x.shape, dtype=F64)
    if int(valid.sum()) == 0:
        return 0.0, grad, 0
    lab = (t[valid] > 0.5).to(dtype)
    e, val, d = _errors(x[valid].to(dtype), lab, kind)
    order = torch.sort(e, descending=True, stable=True).indices
    g = jaccard_gradient(lab[order], dtype)
    gv = torch.zeros(e.shape, dtype=F64)
    gv[order] = (d[order] * g).double()
    grad[valid] = gv
    return float((val[order] * g).double().sum()), grad, int(lab.sum())


def hinge(z, t, per_image=True, ignore=None, loss_scale=1.0, dtype=F64):
    """z, t [B,P] -> (loss, d loss / d z): the mean over the images, or (per_image=False) the one row of the whole batch"""
    B, P = z.shape
    zr, tr = (z, t) if per_image else (z.reshape(1, -1), t.reshape(1, -1))
    R = zr.shape[0]
    out = [row(zr[r], tr[r], ignore, 'hinge', dtype) for r in range(R)]
    loss = sum(o[0] for o in out) / R * loss_scale
    return loss, torch.stack([o[1] for o in out]).reshape(B, P) * loss_scale / R


def softmax_rows(p, t, per_image):
    """[(x, t)] of the class rows in groups of C: per image (b, c) -> plane [HW]; batch-flat c -> the B planes of class c in view(-1) order"""
    B, C, HW = p.shape
    if per_image:
        return [[(p[b, c], t[b, c]) for c in range(C)] for b in range(B)]
    return [[(p[:, c].reshape(-1), t[:, c].reshape(-1)) for c in range(C)]]


def softmax(p, t, only_present=False, per_image=True, ignore=None, loss_scale=1.0, dtype=F64):
    """p, t [B,C,HW] -> (loss, d loss / d p): the mean over the groups (images, or the batch) of the mean over the group's classes, all
    of them or (only_present) those with a positive among the valid elements; a group without such a class adds 0"""
    B, C, HW = p.shape
    groups = softmax_rows(p, t, per_image)
    grad = torch.zeros(p.shape, dtype=F64)
    total = 0.0
    for gi, rows in enumerate(groups):
        out = [row(x, tt, ignore, 'abs', dtype) for x, tt in rows]
        keep = [c for c in range(C) if not only_present or out[c][2] > 0]
        for c in keep:
            total += out[c][0] / len(keep)
            gr = out[c][1] * loss_scale / (len(groups) * len(keep))
            if per_image:
                grad[gi, c] = gr
            else:
                grad[:, c] = gr.reshape(B, HW)
    return total / len(groups) * loss_scale, grad


# ------------------------------------------------------------------------------------------------ the same through autograd
def _row_autograd(x, t, ignore, kind):
    valid = torch.ones_like(t, dtype=torch.bool) if ignore is None else (t != ignore)
    if int(valid.sum()) == 0:
        return x.sum() * 0.0, 0
    lab = (t[valid] > 0.5).to(x.dtype)
    e, val, _ = _errors(x[valid], lab, kind)
    order = torch.sort(e.detach(), descending=True, stable=True).indices
    return (val[order] * jaccard_gradient(lab[order], x.dtype)).sum(), int(lab.sum())


def hinge_autograd(z, t, per_image=True, ignore=None):
    zr, tr = (z, t) if per_image else (z.reshape(1, -1), t.reshape(1, -1))
    return sum(_row_autograd(zr[r], tr[r], ignore, 'hinge')[0] for r in range(zr.shape[0])) / zr.shape[0]


def softmax_autograd(p, t, only_present=False, per_image=True, ignore=None):
    groups = softmax_rows(p, t, per_image)
    total = p.sum() * 0.0
    for rows in groups:
        out = [_row_autograd(x, tt, ignore, 'abs') for x, tt in rows]
        keep = [o for o in out if not only_present or o[1] > 0]
        for o in keep:
            total = total + o[0] / len(keep)
    return total / len(groups)


# ------------------------------------------------------------------------------------------------ cases of the GPU tests
def hinge_case(B, P, void=None):
    """(z, t) float64 [B,P]: logits that are multiples of 1/2 in [-4,4] (every error is exact in fp32, ties abound, so the stable order
    is the only valid one; z = +-1 gives errors of exactly 0), labels in {0,1}.  void: None | 'some' (about 30 % of image 0 and the last
    element of the batch) | 'image' (all of image 0) | 'single' (image 0 keeps one valid element) | 'three' (three elements of image 0)."""
    g = gen('lovasz options hinge', B, P, void)
    z = torch.randint(-8, 9, (B, P), generator=g).to(F64) / 2
    t = (torch.randint(0, POSITIVE_ONE_IN, (B, P), generator=g) == 0).to(F64)
    if P >= 2:                                                  # a forced tie and an error of exactly 0
        z[-1, 1], t[-1, 1] = z[-1, 0], t[-1, 0]
        z[-1, -1], t[-1, -1] = 1.0, 1.0
    return z, put_void(t, void, g)


def put_void(t, void, g):
    """t [B, ...]: write VOID into image 0 (and for 'some' the last element of the batch) as `void` names"""
    t = t.clone()
    flat0 = t[0].reshape(-1)
    n = flat0.numel()
    if void == 'some':
        flat0[torch.rand(n, generator=g) < 0.3] = VOID
        t.reshape(-1)[-1] = VOID
    elif void == 'image':
        flat0[:] = VOID
    elif void == 'single':
        keep = flat0[n // 2].clone()
        flat0[:] = VOID
        flat0[n // 2] = keep
    elif void == 'three':
        flat0[torch.tensor([0, n // 2, n - 1])] = VOID
    t[0] = flat0.reshape(t[0].shape)
    return t


def softmax_case(B, C, HW, void=None, absent=None):
    """(p, t) float64 [B,C,HW]: probabilities that are multiples of 1/32 in [0,1], a random one-hot target, one error of exactly 0 and
    (rows of two elements or more) one forced tie.  absent: None | 'image' (class C-1 has no pixel in image 0) | 'batch' (in no image).
    void as hinge_case, written into every plane of the pixel."""
    g = gen('lovasz options softmax', B, C, HW, void, absent)
    p = torch.randint(0, 33, (B, C, HW), generator=g).to(F64) / 32
    y = torch.randint(0, C, (B, HW), generator=g)
    y[torch.randint(0, POSITIVE_ONE_IN, (B, HW), generator=g) != 0] = 0        # foreground classes share one pixel in POSITIVE_ONE_IN
    if absent == 'image':
        y[0][y[0] == C - 1] = 0
    elif absent == 'batch':
        y[y == C - 1] = 0
    t = F.one_hot(y, C).permute(0, 2, 1).to(F64).contiguous()
    p[B - 1, 0, HW - 1] = t[B - 1, 0, HW - 1]
    if HW >= 2:
        same = t[B - 1, C - 1, 0] == t[B - 1, C - 1, 1]
        p[B - 1, C - 1, 1] = p[B - 1, C - 1, 0] if same else 1.0 - p[B - 1, C - 1, 0]
    if void is not None:
        mark = put_void(torch.zeros(B, HW, dtype=F64), void, g) == VOID
        t = torch.where(mark[:, None, :], torch.full_like(t, VOID), t)
    return p, t


def has_tie(e):
    return int(torch.unique(e).numel()) < e.numel()
