"""TEST HELPER: nn.SyncBatchNorm in train mode, restated in float64 on a list of shards.

What W ranks compute together (processors/ddp_pose_resnet_solver.py:89-90: SyncBatchNorm.convert_sync_batchnorm), written the way the kernel chain
is cut: per-shard sums, their sum over the shards, one finalisation over `total_rows`, a per-shard map; backward the same way round.  Shard i is
z_i [rows_i, C]; every tensor is float64 and stays on the CPU.  tests/test_syncbn_ref_host.py proves this file against torch.nn.BatchNorm2d on the
concatenated batch; tests/test_gpu_syncbn_chain.py compares the kernels with it and with nothing else.
"""
from typing import List, Optional, Sequence

import torch


def _f64(t):
    return None if t is None else t.detach().double().cpu()


def shard_sums(z: torch.Tensor) -> torch.Tensor:
    """One shard's forward message: [C, 2] = (sum, sum of squares) per channel."""
    z = _f64(z)
    return torch.stack((z.sum(0), (z * z).sum(0)), dim=1)


def forward(shards: Sequence[torch.Tensor], gamma, beta, eps: float, momentum: float, running_mean=None, running_var=None,
            residuals: Optional[Sequence[Optional[torch.Tensor]]] = None, relu: bool = False) -> dict:
    """-> dict(local_sums [W][C,2], sums [C,2], total_rows, mean, var (biased), invstd, running_mean, running_var (None without start values),
    pre [W] (before the ReLU), y [W])."""
    zs = [_f64(z) for z in shards]
    gamma, beta = _f64(gamma), _f64(beta)
    local = [shard_sums(z) for z in zs]
    sums = torch.stack(local).sum(0)
    total = sum(z.shape[0] for z in zs)
    mean = sums[:, 0] / total
    var = sums[:, 1] / total - mean * mean                   # biased
    invstd = 1.0 / torch.sqrt(var + eps)
    out = dict(local_sums=local, sums=sums, total_rows=total, mean=mean, var=var, invstd=invstd, running_mean=None, running_var=None)
    if running_mean is not None:
        unbiased = var * total / (total - 1) if total > 1 else var
        out["running_mean"] = (1.0 - momentum) * _f64(running_mean) + momentum * mean
        out["running_var"] = (1.0 - momentum) * _f64(running_var) + momentum * unbiased
    pre = []
    for i, z in enumerate(zs):
        p = (z - mean) * invstd * gamma + beta
        if residuals is not None and residuals[i] is not None:
            p = p + _f64(residuals[i])
        pre.append(p)
    out["pre"] = pre
    out["y"] = [torch.relu(p) if relu else p for p in pre]
    return out


def backward(shards: Sequence[torch.Tensor], dys: Sequence[torch.Tensor], mean, invstd, gamma,
             masks: Optional[Sequence[Optional[torch.Tensor]]] = None) -> dict:
    """`masks[i]` (None: no ReLU) is 1 where shard i's output passed the ReLU.  mean / invstd: the GLOBAL statistics.
    -> dict(g [W], local_dbeta [W][C], local_dgamma [W][C], dbeta [C], dgamma [C], total_rows, dz [W], dres [W])."""
    zs, mean, invstd, gamma = [_f64(z) for z in shards], _f64(mean), _f64(invstd), _f64(gamma)
    gs: List[torch.Tensor] = []
    for i, dy in enumerate(dys):
        g = _f64(dy)
        if masks is not None and masks[i] is not None:
            g = g * _f64(masks[i])
        gs.append(g)
    xhat = [(z - mean) * invstd for z in zs]
    local_dbeta = [g.sum(0) for g in gs]
    local_dgamma = [(g * xh).sum(0) for g, xh in zip(gs, xhat)]
    dbeta, dgamma = torch.stack(local_dbeta).sum(0), torch.stack(local_dgamma).sum(0)
    total = sum(z.shape[0] for z in zs)
    dz = [gamma * invstd * (g - dbeta / total - xh * dgamma / total) for g, xh in zip(gs, xhat)]
    return dict(g=gs, local_dbeta=local_dbeta, local_dgamma=local_dgamma, dbeta=dbeta, dgamma=dgamma, total_rows=total, dz=dz, dres=gs)
