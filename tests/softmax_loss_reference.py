"""Float64 references of the softmax head's operators (csrc/loss_softmax.hip), written for this project from the semantics DESIGN.md pins:
softmax and its Jacobian, the per-(image, class) Lovasz-softmax in closed form (loss and gradient with respect to the probabilities),
Dice + cross entropy in closed form, the same two losses through torch autograd for the CPU cross-checks, and the exactly
representable Lovasz-softmax cases the GPU tests sort.

Importable without a GPU and without the built library."""
import zlib

import torch
import torch.nn.functional as F

F64 = torch.float64

# salt_lovasz_softmax cases of the GPU test: B = 2, C in {2, 3}, every HW below (1 / 2: the smallest rows; 4095 / 4096 / 4097: around the
# first size of the split form; 6145: a last segment of one element)
LOVASZ_B = 2
LOVASZ_C = (2, 3)
LOVASZ_HW = (1, 2, 255, 4095, 4096, 4097, 6145)


def gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


# ------------------------------------------------------------------------------------------------ softmax
def softmax(z):
    """z [B,C,HW] float64 -> p, the pixel's maximum subtracted first"""
    e = torch.exp(z - z.max(1, keepdim=True).values)
    return e / e.sum(1, keepdim=True)


def softmax_bwd(p, dp):
    """dz_j = p_j (dp_j - sum_c p_c dp_c)"""
    return p * (dp - (p * dp).sum(1, keepdim=True))


# ------------------------------------------------------------------------------------------------ Lovasz-softmax
def jaccard_gradient(fg_sorted):
    """g_k = J_k - J_(k-1) of a sorted 0/1 vector (float64): J_k = 1 - (G - c_k) / (G + k - c_k), c_k the positives among the first k"""
    G = fg_sorted.sum()
    inter = G - fg_sorted.cumsum(0)
    union = G + (1.0 - fg_sorted).cumsum(0)
    jac = 1.0 - inter / union
    g = jac.clone()
    g[1:] = jac[1:] - jac[:-1]
    return g


def stable_order(e):
    """descending order of e with ties in ascending index order"""
    return torch.sort(e, descending=True, stable=True).indices


def lovasz_softmax(p, t, loss_scale=1.0):
    """p, t [B,C,HW] float64 -> (loss, d loss / d p, rows [B*C]): closed form, per image and class, all classes, no ignore label.
    The gradient is (fg ? -1 : +1) g_rank loss_scale / (B C) and exactly 0 where the error is 0."""
    B, C, HW = p.shape
    rows = torch.zeros(B * C, dtype=F64)
    grad = torch.zeros_like(p)
    for b in range(B):
        for c in range(C):
            fg = (t[b, c] > 0.5).to(F64)
            e = (fg - p[b, c]).abs()
            order = stable_order(e)
            g = jaccard_gradient(fg[order])
            rows[b * C + c] = (e[order] * g).sum()
            sign = torch.where(fg > 0.5, -1.0, 1.0).to(F64)
            sign = torch.where(e == 0, torch.zeros_like(sign), sign)
            grad[b, c, order] = sign[order] * g * loss_scale / (B * C)
    return float(rows.mean() * loss_scale), grad, rows


def lovasz_softmax_autograd(p, t, loss_scale=1.0):
    """the same loss as a differentiable torch expression of p (the Lovasz extension: the sorted errors dotted with a constant g)"""
    B, C, HW = p.shape
    total = p.new_zeros(())
    for b in range(B):
        for c in range(C):
            fg = (t[b, c] > 0.5).to(F64)
            e = (fg - p[b, c]).abs()
            order = stable_order(e.detach())
            total = total + (e[order] * jaccard_gradient(fg[order])).sum()
    return total * loss_scale / (B * C)


def lovasz_case(C, HW, B=LOVASZ_B):
    """(p, t) float64 [B,C,HW]: probabilities that are multiples of 1/32 in [0,1] (every error is exact in fp32, so the stable order is
    the only valid one; the channels need not sum to 1), a random one-hot target whose image 0 is all background, one error of exactly
    0, and - where a row has two elements - one forced tie."""
    g = gen('lovasz_softmax', C, HW)
    p = torch.randint(0, 33, (B, C, HW), generator=g).to(F64) / 32
    y = torch.randint(0, C, (B, HW), generator=g)
    y[0] = 0                                                   # image 0: every foreground channel is all zero
    t = F.one_hot(y, C).permute(0, 2, 1).to(F64).contiguous()
    p[B - 1, 0, HW - 1] = t[B - 1, 0, HW - 1]                  # an error of exactly 0
    if HW >= 2:                                                # elements 0 and 1 of the last row tie
        same = t[B - 1, C - 1, 0] == t[B - 1, C - 1, 1]
        p[B - 1, C - 1, 1] = p[B - 1, C - 1, 0] if same else 1.0 - p[B - 1, C - 1, 0]
    return p, t


def tie_groups(p, t):
    """number of rows (b, c) that hold at least two equal errors, and the number of errors that are exactly 0"""
    e = ((t > 0.5).to(F64) - p).abs()
    rows = sum(int(torch.unique(e[b, c]).numel() < e.shape[2]) for b in range(e.shape[0]) for c in range(e.shape[1]))
    return rows, int((e == 0).sum())


# ------------------------------------------------------------------------------------------------ Dice + cross entropy
def dice_ce(z, t, dice_weight=0.5, cross_entropy_weight=0.5, smooth=0.0, loss_scale=1.0):
    """z, t [B,C,HW] float64 -> (loss, d loss / d z, sums [3C+1]): closed form.  sums: per class (sum p t, sum p, sum t), then the
    cross-entropy sum.  Dice over the classes 1 .. C-1 with batch-wide sums; the label is the target's first maximum."""
    B, C, HW = z.shape
    N = B * HW
    m = z.max(1, keepdim=True).values
    lse = m + torch.log(torch.exp(z - m).sum(1, keepdim=True))
    p = torch.exp(z - lse)
    y = t.argmax(1)                                            # first maximum
    onehot = F.one_hot(y, C).permute(0, 2, 1).to(F64)
    ce_sum = (lse[:, 0] - z.gather(1, y[:, None])[:, 0]).sum()
    I, P, T = (p * t).sum((0, 2)), p.sum((0, 2)), t.sum((0, 2))
    D = P + T + smooth + 1e-7
    dice = (1.0 - (2.0 * I + smooth) / D)[1:].sum()
    loss = loss_scale * (dice_weight * dice / (C - 1) + cross_entropy_weight * ce_sum / N)
    dp = dice_weight / (C - 1) * (-2.0 * t / D[None, :, None] + ((2.0 * I + smooth) / D ** 2)[None, :, None])
    dp[:, 0] = 0.0
    dz = loss_scale * (softmax_bwd(p, dp) + cross_entropy_weight / N * (p - onehot))
    sums = torch.cat([torch.stack([I, P, T], 1).reshape(-1), ce_sum.reshape(1)])
    return float(loss), dz, sums


def dice_ce_autograd(z, t, dice_weight=0.5, cross_entropy_weight=0.5, smooth=0.0, loss_scale=1.0):
    """the same loss from F.cross_entropy and the Dice formula on F.softmax, differentiable in z"""
    B, C, HW = z.shape
    p = F.softmax(z, 1)
    ce = F.cross_entropy(z, t.argmax(1))
    dice = z.new_zeros(())
    for c in range(1, C):
        inter = (p[:, c] * t[:, c]).sum()
        dice = dice + 1.0 - (2.0 * inter + smooth) / (p[:, c].sum() + t[:, c].sum() + smooth + 1e-7)
    return loss_scale * (dice_weight * dice / (C - 1) + cross_entropy_weight * ce)


def random_target(shape, g, kind='random'):
    """one-hot float64 [B,C,HW]; 'background': every pixel is class 0"""
    B, C, HW = shape
    y = torch.randint(0, C, (B, HW), generator=g) if kind == 'random' else torch.zeros((B, HW), dtype=torch.int64)
    return F.one_hot(y, C).permute(0, 2, 1).to(F64).contiguous()


def large_logits(shape, g):
    return torch.tensor([-80.0, -15.0, 0.0, 15.0, 80.0], dtype=F64)[torch.randint(0, 5, shape, generator=g)]
