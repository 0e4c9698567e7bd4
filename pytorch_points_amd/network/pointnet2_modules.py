"""Drop-in for ``pytorch_points.network.pointnet2_modules``: the PointNet++ set-abstraction and feature-propagation
modules.  Compositions of operators this package already serves -- the fused ``QueryAndGroup``, ``GroupAll``,
``furthest_point_sample(..., NCHW=False)``, ``three_nn`` and ``three_interpolate`` -- with the reference's signatures,
defaults and ``state_dict()`` keys (network/pointnet2_modules.py); the code is this package's own.

Quirks of the reference that run there and are kept: with ``use_xyz`` the constructor adds 3 to the first entry of the
CALLER's ``mlp`` list, and ``bn`` is accepted and ignored (``normalization`` decides)."""
import torch
import torch.nn.functional as F
from torch import nn

from . import pointnet2_utils
from .geo_operations import furthest_point_sample
from .layers import SharedMLP
from .operations import QueryAndGroup


class _PointnetSAModuleBase(nn.Module):

    def __init__(self):
        super().__init__()
        self.npoint = None
        self.groupers = None
        self.mlps = None
        self.pool_method = "max_pool"

    def forward(self, xyz, features=None, new_xyz=None):
        """xyz (B,N,3), features (B,C,N) or None, new_xyz (B,npoint,3) or None: sampled here from ``xyz``
        -> (new_xyz (B,npoint,3) -- None when the whole cloud is one group --, new_features (B, sum of the scales'
        last widths, npoint))"""
        if new_xyz is None and self.npoint is not None:
            new_xyz = furthest_point_sample(xyz, self.npoint, NCHW=False)[1]
        pooled = []
        for grouper, mlp in zip(self.groupers, self.mlps):
            grouped = mlp(grouper(xyz, new_xyz, features))            # (B, mlp[-1], npoint, nsample)
            window = [1, grouped.size(3)]
            if self.pool_method == "max_pool":
                grouped = F.max_pool2d(grouped, kernel_size=window)
            elif self.pool_method == "avg_pool":
                grouped = F.avg_pool2d(grouped, kernel_size=window)
            else:
                raise NotImplementedError
            pooled.append(grouped.squeeze(-1))
        return new_xyz, torch.cat(pooled, dim=1)


class PointnetSAModuleMSG(_PointnetSAModuleBase):
    """Set abstraction with multi-scale grouping: one ball query and one SharedMLP per radius.  ``npoint`` None: the
    whole cloud is one group (GroupAll)."""

    def __init__(self, *, npoint, radii, nsamples, mlps, bn=True, use_xyz=True, pool_method="max_pool",
                 normalization="batch"):
        super().__init__()
        assert len(radii) == len(nsamples) == len(mlps)
        self.npoint = npoint
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for radius, nsample, mlp_spec in zip(radii, nsamples, mlps):
            self.groupers.append(QueryAndGroup(radius, nsample, use_xyz=use_xyz) if npoint is not None
                                 else pointnet2_utils.GroupAll(use_xyz))
            if use_xyz:
                mlp_spec[0] += 3          # the caller's list, as in the reference
            self.mlps.append(SharedMLP(mlp_spec, normalization=normalization, activation="relu"))
        self.pool_method = pool_method


class PointnetSAModule(PointnetSAModuleMSG):
    """Set abstraction at one scale."""

    def __init__(self, *, mlp, npoint=None, radius=None, nsample=None, bn=True, use_xyz=True, pool_method="max_pool",
                 normalization="batch"):
        super().__init__(mlps=[mlp], npoint=npoint, radii=[radius], nsamples=[nsample], bn=bn, use_xyz=use_xyz,
                         pool_method=pool_method, normalization=normalization)


class PointnetFPModule(nn.Module):
    """Feature propagation: the known features interpolated to the unknown points (inverse-distance weights over the
    three nearest known points), concatenated with the unknown points' own features, through a SharedMLP."""

    def __init__(self, *, mlp, normalization="batch"):
        super().__init__()
        self.mlp = SharedMLP(mlp, normalization=normalization, activation="relu")

    def forward(self, unknown, known, unknow_feats, known_feats):
        """unknown (B,n,3), known (B,m,3) or None (``known_feats`` (B,C2,1) is then repeated), unknow_feats (B,C1,n)
        or None, known_feats (B,C2,m) -> (B, mlp[-1], n)"""
        if known is not None:
            dist, idx = pointnet2_utils.three_nn(unknown, known)
            dist_recip = 1.0 / (dist + 1e-8)
            weight = dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)
            interpolated = pointnet2_utils.three_interpolate(known_feats, idx, weight)
        else:
            interpolated = known_feats.expand(*known_feats.size()[0:2], unknown.size(1))
        if unknow_feats is not None:
            interpolated = torch.cat([interpolated, unknow_feats], dim=1)
        return self.mlp(interpolated.unsqueeze(-1)).squeeze(-1)
