"""tests/syncbn_ref.py (the float64 restatement of the SyncBatchNorm chain that tests/test_gpu_syncbn_chain.py measures the kernels against) proved
against torch.nn.BatchNorm2d in float64 train mode on the CONCATENATED batch: outputs, the running statistics after one step from non-trivial
start values, and autograd's dz / dgamma / dbeta / dres, for 1, 2 and 3 shards of unequal size.  The bar is float64's own rounding.  No GPU.

Also here, because it needs no GPU either: every BatchNorm width of every net factory passes the width condition of the reduction kernels
(include/simple_pose_hip.h next to SP_REDUCE_WORKSPACE_BYTES)."""
import pytest
import torch

from tests import syncbn_ref as ref

EPS, MOMENTUM = 1e-5, 0.1
BAR = 1e-12
SHARDS = [(41,), (300, 1), (37, 64, 5)]


def _rel(got, want):
    return float((got - want).abs().max() / want.pow(2).mean().sqrt())


def _operands(rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    scale, shift = 0.5 + torch.rand(C, generator=g, dtype=torch.float64), r(C)
    zs = [r(n, C) * scale + shift for n in rows]
    ress = [r(n, C) for n in rows]
    dys = [r(n, C) for n in rows]
    gamma, beta = 0.75 + 0.5 * torch.rand(C, generator=g, dtype=torch.float64), 0.1 * r(C)
    rm0, rv0 = r(C), 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    return zs, ress, dys, gamma, beta, rm0, rv0


@pytest.mark.parametrize("relu,res_on", [(False, False), (True, False), (True, True), (False, True)], ids=["plain", "relu", "res_relu", "res"])
@pytest.mark.parametrize("rows", SHARDS, ids=lambda r: "x".join(map(str, r)))
def test_sharded_float64_chain_equals_batchnorm2d_on_the_concatenated_batch(rows, relu, res_on):
    C = 24
    zs, ress, dys, gamma, beta, rm0, rv0 = _operands(rows, C, seed=sum(rows) + C)
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOMENTUM).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
    z_all = torch.cat(zs).clone().requires_grad_(True)
    r_all = torch.cat(ress).clone().requires_grad_(True)
    pre = bn(z_all.view(-1, C, 1, 1)).view(-1, C)
    if res_on:
        pre = pre + r_all
    y = torch.relu(pre) if relu else pre
    (y * torch.cat(dys)).sum().backward()
    # one mask for both sides: where torch's own output passed the ReLU
    masks = [(m > 0).double() for m in y.detach().split(list(rows))] if relu else None

    f = ref.forward(zs, gamma, beta, EPS, MOMENTUM, rm0, rv0, residuals=ress if res_on else None, relu=relu)
    assert f["total_rows"] == sum(rows)
    assert _rel(torch.cat(f["y"]), y.detach()) <= BAR
    assert _rel(f["running_mean"], bn.running_mean) <= BAR and _rel(f["running_var"], bn.running_var) <= BAR
    z64 = torch.cat(zs)
    assert _rel(f["mean"], z64.mean(0)) <= BAR and _rel(f["invstd"], 1 / torch.sqrt(z64.var(0, unbiased=False) + EPS)) <= BAR
    assert torch.equal(f["sums"], torch.stack(f["local_sums"]).sum(0)) and len(f["local_sums"]) == len(rows)

    b = ref.backward(zs, dys, f["mean"], f["invstd"], gamma, masks)
    assert _rel(torch.cat(b["dz"]), z_all.grad) <= BAR
    assert _rel(b["dgamma"], bn.weight.grad) <= BAR and _rel(b["dbeta"], bn.bias.grad) <= BAR
    if res_on:
        assert _rel(torch.cat(b["dres"]), r_all.grad) <= BAR
    # the parameter gradients are the sum of the local ones, and a local one is that shard's own sum
    assert _rel(torch.stack(b["local_dgamma"]).sum(0), bn.weight.grad) <= BAR
    assert torch.equal(b["local_dbeta"][0], b["g"][0].sum(0))


def test_the_restatement_tells_global_statistics_from_per_shard_ones():
    """What the GPU tests rely on the reference to see: statistics over one shard instead of the whole batch, the biased variance in the running
    statistics, and momentum swapped with 1 - momentum all move the result by far more than any bar in use."""
    rows, C = (37, 64, 5), 24
    zs, _, _, gamma, beta, rm0, rv0 = _operands(rows, C, seed=3)
    f = ref.forward(zs, gamma, beta, EPS, MOMENTUM, rm0, rv0)
    alone = ref.forward(zs[:1], gamma, beta, EPS, MOMENTUM, rm0, rv0)
    assert _rel(alone["mean"], f["mean"]) > 1e-2 and _rel(alone["y"][0], f["y"][0]) > 1e-2
    n = f["total_rows"]
    biased = (1 - MOMENTUM) * rv0 + MOMENTUM * f["var"]
    assert _rel(biased, f["running_var"]) > 0.2 * MOMENTUM / n
    swapped = ref.forward(zs, gamma, beta, EPS, 1 - MOMENTUM, rm0, rv0)
    assert _rel(swapped["running_mean"], f["running_mean"]) > 0.1


def test_every_batchnorm_width_of_every_net_passes_the_reduction_width_condition():
    """c/4 <= 256 or c/4 a multiple of 256: no net of the repository has a BatchNorm the reduction entry points would refuse (and the widest
    one, 2048 channels, is the two-trip case the GPU tests run)."""
    import os
    from simple_pose_amd import nets
    from simple_pose_amd.nets import pose_hrnet, pose_resnet_dconv, pose_resnet_duc
    built = []
    with torch.device("meta"):
        for mod in (pose_resnet_dconv, pose_resnet_duc):
            built += [getattr(mod, name)(pretrained=False) for name in mod.__all__ if name != "ResNet"]
        here = os.path.dirname(nets.__file__)
        built += [pose_hrnet.get_pose_net(os.path.join(here, cfg)) for cfg in ("hrnet_w32.yaml", "hrnet_w48.yaml")]
    widths = {v.shape[0] for net in built for k, v in net.state_dict().items() if k.endswith("running_mean")}
    print(len(built), "nets; BatchNorm widths", sorted(widths))
    assert len(built) >= 20 and {64, 384, 2048} <= widths
    refused = sorted(c for c in widths if c % 4 or not (c // 4 <= 256 or (c // 4) % 256 == 0))
    assert not refused, refused
