"""Drop-in for ``pytorch_points.network.layers``: SharedMLP, the Conv2d / Conv1d / Linear wrappers with a
normalisation and an activation, ShuffleBlock, DenseEdgeConv and SampledDenseEdgeConv.  Constructor and ``forward``
signatures, defaults, error messages and ``state_dict()`` keys follow the reference (network/layers.py), so that its
checkpoints load; the code is this package's own.

The two EdgeConv modules build their edge tensor ``[x_i, x_j - x_i]`` with ``edge_features.knn_edge_features`` (one HIP
kernel that writes it once) where the reference gathers, permutes, slices, expands and concatenates; ``forward_unfused``
keeps that composition as the yardstick of the tests and of tools/edge_features_time.py.  Differences from the
reference, both where its code does not run: ``DenseEdgeConv.forward(x, idx=given)`` gathers with the
given graph (a NameError there), and ``SampledDenseEdgeConv`` unpacks ``knn_points``' three results correctly (a
ValueError there)."""
import torch
from torch import nn

from .. import edge_features, ops
from .geo_operations import furthest_point_sample
from .operations import gather_points


def _norm_act(module, normalization, activation, momentum, batch_norm, instance_norm, channels):
    """the part the three wrappers share: ``module.norm`` and ``module.act``, where asked for"""
    module.activation = activation
    module.normalization = normalization
    if normalization is not None:
        if normalization == "batch":
            module.norm = batch_norm(channels, affine=True, eps=0.001, momentum=momentum)
        elif normalization == "instance":
            module.norm = instance_norm(channels, affine=True, eps=0.001, momentum=momentum)
        else:
            raise ValueError("only \"batch/instance\" normalization permitted.")
    if activation is not None:
        if activation == "relu":
            module.act = nn.ReLU()
        elif activation == "elu":
            module.act = nn.ELU(alpha=1.0)
        elif activation == "lrelu":
            module.act = nn.LeakyReLU(0.1)
        elif activation == "tanh":
            module.act = nn.Tanh()
        else:
            raise ValueError("only \"relu/elu/lrelu/tanh\" implemented")


def _apply_norm_act(module, x):
    if module.normalization is not None:
        x = module.norm(x)
    if module.activation is not None:
        x = module.act(x)
    return x


class Conv2d(nn.Module):
    """2-D convolution, then the normalisation ("batch" / "instance") and the activation asked for.  With a
    normalisation the convolution has no bias."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, activation=None,
                 normalization=None, momentum=0.01, conv_params={}):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding,
                              bias=bool(not normalization and bias), **conv_params)
        _norm_act(self, normalization, activation, momentum, nn.BatchNorm2d, nn.InstanceNorm2d, out_channels)

    def forward(self, x, epoch=None):
        return _apply_norm_act(self, self.conv(x))


class Conv1d(nn.Module):
    """1-D convolution, then the normalisation and the activation asked for."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, activation=None,
                 normalization=None, momentum=0.01, conv_params={}):
        super().__init__()
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size, stride=stride, padding=padding,
                              bias=bool(not normalization and bias), **conv_params)
        _norm_act(self, normalization, activation, momentum, nn.BatchNorm1d, nn.InstanceNorm1d, out_channels)

    def forward(self, x, epoch=None):
        return _apply_norm_act(self, self.conv(x))


class Linear(nn.Module):
    """Linear layer, then the normalisation and the activation asked for."""

    def __init__(self, in_channels, out_channels, bias=True, activation=None, normalization=None, momentum=0.01):
        super().__init__()
        self.linear = nn.Linear(in_channels, out_channels, bias=bool(not normalization and bias))
        _norm_act(self, normalization, activation, momentum, nn.BatchNorm1d, nn.InstanceNorm1d, out_channels)

    def forward(self, x, epoch=None):
        return _apply_norm_act(self, self.linear(x))


class SharedMLP(nn.Sequential):
    """1x1 ``Conv2d`` wrappers ``layer0``, ``layer1``, ... over the channel counts ``args``."""

    def __init__(self, args, activation=None, normalization=None, **kwargs):
        super().__init__()
        for i in range(len(args) - 1):
            self.add_module("layer{}".format(i),
                            Conv2d(args[i], args[i + 1], 1, normalization=normalization, activation=activation))


class ShuffleBlock(nn.Module):
    """Channel shuffle of (N,C,H,W): the channels of the ``groups`` groups interleaved."""

    def __init__(self, groups=2):
        super().__init__()
        self.groups = groups

    def forward(self, x):
        n, c, h, w = x.size()
        g = self.groups
        return x.view(n, g, c // g, h, w).permute(0, 2, 1, 3, 4).reshape(n, c, h, w)


def _search(centres, x, k):
    """``(B,P,k)``: the k nearest columns of ``x`` (B,C,N) to every column of ``centres`` (B,C,P) behind the nearest
    one (the centre itself, where it is a column of ``x``).  The search runs in fp32 and outside autograd: its
    distances are not used."""
    with torch.no_grad():
        a = centres.detach().transpose(1, 2).float()
        b = a if centres is x else x.detach().transpose(1, 2).float()
        return ops.knn_points(a, b, K=k + 1).idx[:, :, 1:]


def _edges_unfused(centres, x, idx):
    """the edge tensor the reference's way: ``knn_gather`` (B,P,K,C), permute, expand, concatenate"""
    nb = ops.knn_gather(x.transpose(1, 2), idx.long()).permute(0, 3, 1, 2)
    centre = centres.unsqueeze(-1).expand_as(nb)
    return torch.cat([centre, nb - centre], dim=1)


class DenseEdgeConv(nn.Module):
    """Densely connected EdgeConv: ``n`` 1x1 convolutions of ``growth_rate`` channels over the edge features of the
    k-NN graph in feature space, every one fed with all earlier outputs, and a maximum over the k neighbours.

    forward(x (B,C,N), idx=None | (B,N,k)) -> (y (B, C + n * growth_rate, N), idx (B,N,k))"""

    def __init__(self, in_channels, growth_rate, n, k, **kwargs):
        super().__init__()
        self.growth_rate = growth_rate
        self.n = n
        self.k = k
        self.mlps = nn.ModuleList()
        self.mlps.append(nn.Conv2d(2 * in_channels, growth_rate, 1, bias=True))
        for _ in range(1, n):
            in_channels += growth_rate
            self.mlps.append(nn.Conv2d(in_channels, growth_rate, 1, bias=True))
        self.out_channels = in_channels + growth_rate

    def get_local_graph(self, x, k, idx=None, fused=True):
        """``(edge features (B,2C,N,k), idx (B,N,k))`` of ``x`` (B,C,N); ``idx`` None: searched here"""
        if idx is None:
            idx = _search(x, x, k)
        if fused:
            return edge_features.knn_edge_features(x, idx), idx
        return _edges_unfused(x, x, idx), idx

    def _dense(self, y, centres):
        """the dense growth over the edge features ``y``, ``centres`` (B,C,P) repeated along k beside the first
        layer's output, and the maximum over k"""
        for i, mlp in enumerate(self.mlps):
            if i == 0:
                y = torch.cat([nn.functional.relu_(mlp(y)), centres.unsqueeze(-1).expand(-1, -1, -1, self.k)], dim=1)
            elif i == self.n - 1:
                y = torch.cat([mlp(y), y], dim=1)
            else:
                y = torch.cat([nn.functional.relu_(mlp(y)), y], dim=1)
        return torch.max(y, dim=-1)[0]

    def forward(self, x, idx=None):
        y, idx = self.get_local_graph(x, k=self.k, idx=idx)
        return self._dense(y, x), idx

    def forward_unfused(self, x, idx=None):
        """``forward`` with the edge tensor composed the reference's way: the yardstick of the parity tests and of
        tools/edge_features_time.py"""
        y, idx = self.get_local_graph(x, k=self.k, idx=idx, fused=False)
        return self._dense(y, x), idx


class SampledDenseEdgeConv(DenseEdgeConv):
    """DenseEdgeConv at ``nsample`` centres picked from the cloud: furthest point sampling of ``xyz`` (B,3,N), or for
    ``nsample == 1`` the point nearest to the centroid.

    forward(x (B,C,N), nsample, xyz (B,3,N)) -> (y (B,C',nsample), sampled_xyz, sampled_idx (B,nsample));
    sampled_xyz is (B,3,nsample) from the sampling and (B,1,3) for ``nsample == 1``, as in the reference."""

    def get_local_graph(self, query, x, k, idx=None, fused=True):
        """``(edge features (B,2C,P,k), idx (B,P,k))`` of the centres ``query`` (B,C,P) over ``x`` (B,C,N)"""
        if idx is None:
            idx = _search(query, x, k)
        if fused:
            return edge_features.knn_edge_features(x, idx, query), idx
        return _edges_unfused(query, x, idx), idx

    def _sample(self, x, nsample, xyz):
        if nsample == 1:
            centroid = torch.mean(xyz, dim=-1, keepdim=True)
            _, sampled_idx, sampled_xyz = ops.knn_points(centroid.transpose(1, 2), xyz.transpose(1, 2), return_nn=True)
            sampled_xyz = sampled_xyz.squeeze(2)
            sampled_idx = sampled_idx.squeeze(1)
        else:
            sampled_idx, sampled_xyz = furthest_point_sample(xyz, nsample, NCHW=True)
        return gather_points(x, sampled_idx), sampled_xyz, sampled_idx

    def forward(self, x, nsample, xyz):
        sampled_x, sampled_xyz, sampled_idx = self._sample(x, nsample, xyz)
        y, _ = self.get_local_graph(sampled_x, x, k=self.k)
        return self._dense(y, sampled_x), sampled_xyz, sampled_idx

    def forward_unfused(self, x, nsample, xyz):
        sampled_x, sampled_xyz, sampled_idx = self._sample(x, nsample, xyz)
        y, _ = self.get_local_graph(sampled_x, x, k=self.k, fused=False)
        return self._dense(y, sampled_x), sampled_xyz, sampled_idx
