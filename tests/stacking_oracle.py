"""Comparator for the second-level networks (TEST INFRASTRUCTURE ONLY): architectures/misc.py:8-36 (StackingFCN / StackingFCNWithDepth)
restated in plain torch from a state dict.  Runs on whatever device the tensors live on (tools/stacking_bench.py times it on the GPU in
torch eager).  ``bf16=True`` emulates bf16 storage the way oracle.blocks.bf16_storage does: the input maps, the convolution weight, the
raw convolution output and the activation are rounded to bf16, everything else stays fp32."""
import torch
import torch.nn.functional as F


def _r(x, bf16):
    return x.bfloat16().to(x.dtype) if bf16 else x


def batch_norm(sd, p, y, train, momentum=0.1, eps=1e-5):
    """nn.BatchNorm2d with torch defaults; train=True also updates the running statistics in ``sd`` like the module does."""
    if train:
        if (p + 'num_batches_tracked') in sd:
            sd[p + 'num_batches_tracked'] += 1
        return F.batch_norm(y, sd[p + 'running_mean'], sd[p + 'running_var'], sd[p + 'weight'], sd[p + 'bias'], True, momentum, eps)
    return F.batch_norm(y, sd[p + 'running_mean'], sd[p + 'running_var'], sd[p + 'weight'], sd[p + 'bias'], False, momentum, eps)


def depth_gate(sd, d, p='depth_channel_excitation.'):
    """sigmoid(nn.Linear(1, F)(d)) -> [B, F] (architectures/base.py:120-131)"""
    return torch.sigmoid(F.linear(d, sd[p + 'fc.0.weight'], sd[p + 'fc.0.bias']))


def stacking_fcn(sd, x, train, d=None, bf16=False):
    """x [B,M,H,W] (+ d [B,1] for the depth variant: the gate keys decide) -> logits [B,K,H,W].
    base.Conv2dBnRelu: ReplicationPad2d((left 0, right 2, top 2, bottom 0)) -> Conv2d 3x3 pad 0 -> BatchNorm2d -> ReLU; then the gate;
    then the 1x1 head.  F.dropout2d(p=0) of the reference is an identity."""
    xp = F.pad(_r(x, bf16), (0, 2, 2, 0), mode='replicate')
    y = _r(F.conv2d(xp, _r(sd['conv.0.conv.weight'], bf16), sd['conv.0.conv.bias']), bf16)
    a = _r(F.relu(batch_norm(sd, 'conv.0.batch_norm.', y, train)), bf16)
    if 'depth_channel_excitation.fc.0.weight' in sd:
        a = _r(a * depth_gate(sd, d)[:, :, None, None], bf16)
    return F.conv2d(a, sd['final.0.weight'], sd['final.0.bias'])


def state_keys(with_depth):
    keys = ['conv.0.batch_norm.weight', 'conv.0.batch_norm.bias', 'conv.0.batch_norm.running_mean', 'conv.0.batch_norm.running_var',
            'conv.0.batch_norm.num_batches_tracked', 'conv.0.conv.weight', 'conv.0.conv.bias']
    if with_depth:
        keys += ['depth_channel_excitation.fc.0.weight', 'depth_channel_excitation.fc.0.bias']
    return keys + ['final.0.weight', 'final.0.bias']


def lovasz_loss(output, target):
    """models.py:326-328 + lovasz_losses.py:81-115 (per image, F.elu variant), dtype-generic: every image's [K,H,W] logits and one-hot targets are
    flattened together, as the reference's lovasz_hinge does with the 4-d tensors it is handed."""
    vals = []
    for lg, lb in zip(output, target):
        lg, lb = lg.reshape(-1), lb.reshape(-1).to(lg.dtype)
        err = 1.0 - lg * (2.0 * lb - 1.0)
        es, perm = torch.sort(err, dim=0, descending=True)
        gt = lb[perm]
        total = gt.sum()
        jac = 1.0 - (total - gt.cumsum(0)) / (total + (1.0 - gt).cumsum(0))
        if gt.numel() > 1:
            jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        vals.append(torch.dot(F.elu(es), jac))
    return sum(vals) / len(vals)
