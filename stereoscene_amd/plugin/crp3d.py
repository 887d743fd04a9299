"""3-D context relation prior: host-side mirrors of ``Bottleneck3D``, ``Process``, ``ASPP`` and ``CPMegaVoxels``
(occupancy/backbones/crp3d.py:4-262) with identical constructor arguments and state-dict keys.  The convolutions run on the
MFMA kernels (the anisotropic (1,1,3) and the dilated 3x3x3 ones on the generic gather kernel), the BatchNorms on the fused
normalisation kernels with their residual and ReLU, the relation gather on ``functional.relation_gather`` (csrc/crp.hip)."""
import torch
import torch.nn as nn

from .. import functional as F
from ..layers import BatchNorm3d, Conv3d


class Bottleneck3D(nn.Module):
    """crp3d.py:4-108.  Only ``stride == 1`` runs (``CPMegaVoxels`` uses nothing else): the AvgPool shortcuts ``downsample2/3/4``
    keep their parameters under the reference's names and ``forward`` raises for any other stride."""

    def __init__(self, inplanes, planes, norm_layer, stride=1, dilation=[1, 1, 1], expansion=4, downsample=None, fist_dilation=1,
                 multi_grid=1, bn_momentum=0.0003):
        super().__init__()
        self.expansion = expansion
        self.conv1 = Conv3d(inplanes, planes, 1, bias=False)
        self.bn1 = norm_layer(planes, momentum=bn_momentum)
        self.conv2 = Conv3d(planes, planes, (1, 1, 3), (1, 1, stride), (0, 0, dilation[0]), (1, 1, dilation[0]), bias=False)
        self.bn2 = norm_layer(planes, momentum=bn_momentum)
        self.conv3 = Conv3d(planes, planes, (1, 3, 1), (1, stride, 1), (0, dilation[1], 0), (1, dilation[1], 1), bias=False)
        self.bn3 = norm_layer(planes, momentum=bn_momentum)
        self.conv4 = Conv3d(planes, planes, (3, 1, 1), (stride, 1, 1), (dilation[2], 0, 0), (dilation[2], 1, 1), bias=False)
        self.bn4 = norm_layer(planes, momentum=bn_momentum)
        self.conv5 = Conv3d(planes, planes * self.expansion, (1, 1, 1), bias=False)
        self.bn5 = norm_layer(planes * self.expansion, momentum=bn_momentum)
        self.relu = nn.ReLU(inplace=False)
        self.relu_inplace = nn.ReLU(inplace=True)
        self.downsample, self.dilation, self.stride = downsample, dilation, stride

        def shortcut(kernel):
            return nn.Sequential(nn.AvgPool3d(kernel_size=kernel, stride=kernel), Conv3d(planes, planes, 1, 1, bias=False),
                                 norm_layer(planes, momentum=bn_momentum))
        self.downsample2 = shortcut((1, stride, 1))
        self.downsample3 = shortcut((stride, 1, 1))
        self.downsample4 = shortcut((stride, 1, 1))

    def forward(self, x):
        if self.stride != 1 or self.downsample is not None:
            raise NotImplementedError("Bottleneck3D: only stride 1 without a projected shortcut is built (what CPMegaVoxels uses)")
        out1 = self.bn1(self.conv1(x), relu=True)
        out2 = self.bn2(self.conv2(out1), relu=False)
        out3 = self.bn3(self.conv3(torch.relu(out2)), residual=out2, relu=False)
        out4_relu = self.bn4(self.conv4(torch.relu(out3)), residual=out2 + out3, relu=True)
        return self.bn5(self.conv5(out4_relu), residual=x, relu=True)


class Process(nn.Module):
    def __init__(self, feature, norm_layer, bn_momentum, dilations=[1, 2, 3]):
        super().__init__()
        self.main = nn.Sequential(*[Bottleneck3D(feature, feature // 4, bn_momentum=bn_momentum, norm_layer=norm_layer,
                                                 dilation=[i, i, i]) for i in dilations])

    def forward(self, x):
        return self.main(x)


class ASPP(nn.Module):
    """crp3d.py:129-171: relu(sum over the dilations of BN(conv(relu(BN(conv(x))))) + x)."""

    def __init__(self, planes, dilations_conv_list):
        super().__init__()
        self.conv_list = dilations_conv_list
        self.conv1 = nn.ModuleList([Conv3d(planes, planes, 3, 1, d, d, bias=False) for d in dilations_conv_list])
        self.bn1 = nn.ModuleList([BatchNorm3d(planes) for _ in dilations_conv_list])
        self.conv2 = nn.ModuleList([Conv3d(planes, planes, 3, 1, d, d, bias=False) for d in dilations_conv_list])
        self.bn2 = nn.ModuleList([BatchNorm3d(planes) for _ in dilations_conv_list])
        self.relu = nn.ReLU()

    def forward(self, x_in):
        y = None
        for i in range(len(self.conv_list)):                 # y += branch i, in the reference's order
            y = self.bn2[i](self.conv2[i](self.bn1[i](self.conv1[i](x_in), relu=True)), residual=y, relu=False)
        return torch.relu(y + x_in)


class CPMegaVoxels(nn.Module):
    """crp3d.py:173-262.  The four ``context_prior_logits`` convolutions stay four parameters and run as one pointwise layer; its
    channels-last result [B, N, 4, Mc] is handed on as the view ``P_logits`` [B, 4, Mc, N].  sigmoid, the four ``bmm`` and both
    ``cat`` of the reference are one operator (``functional.relation_gather``)."""

    def __init__(self, feature, size, n_relations=4, bn_momentum=0.0003):
        super().__init__()
        self.size, self.n_relations = tuple(size), n_relations
        self.flatten_size = size[0] * size[1] * size[2]
        self.feature, self.context_feature = feature, feature * 2
        padding = ((size[0] + 1) % 2, (size[1] + 1) % 2, (size[2] + 1) % 2)
        self.mega_context = nn.Sequential(Conv3d(feature, self.context_feature, 3, 2, padding))
        self.flatten_context_size = (size[0] // 2) * (size[1] // 2) * (size[2] // 2)
        self.context_prior_logits = nn.ModuleList([nn.Sequential(Conv3d(feature, self.flatten_context_size, 1, 1, 0))
                                                   for _ in range(n_relations)])
        self.aspp = ASPP(feature, [1, 2, 3])
        self.resize = nn.Sequential(Conv3d(self.context_feature * n_relations + feature, feature, 1, 1, 0, bias=False),
                                    Process(feature, BatchNorm3d, bn_momentum, dilations=[1]))

    def forward(self, input):
        if F.storage_bf16() or input.dtype != torch.float32:
            raise NotImplementedError("crp3d=True runs in fp32 only: the relation kernels have no bf16 storage form "
                                      "(set_precision('fp32') or build the encoder with crp3d=False)")
        if tuple(input.shape[2:]) != self.size:
            raise ValueError(f"CPMegaVoxels: built for the grid {self.size} (crp_size), got {tuple(input.shape[2:])}")
        bs, R = input.shape[0], self.n_relations
        x_agg = self.aspp(input)
        ctx = self.mega_context(x_agg)                                               # logical [B, C2, X/2, Y/2, Z/2]
        if ctx[0, 0].numel() != self.flatten_context_size:
            raise ValueError(f"CPMegaVoxels: the mega context has {ctx[0, 0].numel()} voxels, {self.flatten_context_size} expected")
        ctx = ctx.reshape(bs, self.context_feature, -1).permute(0, 2, 1)             # [B, Mc, C2]: its channels-last memory
        w = torch.cat([seq[0].weight for seq in self.context_prior_logits], dim=0)
        b = torch.cat([seq[0].bias for seq in self.context_prior_logits], dim=0)
        p = F.conv3d(x_agg, w, b)                                                    # logical [B, R Mc, X, Y, Z]
        P_logits = p.reshape(bs, R, self.flatten_context_size, self.flatten_size)    # a view: channel = r Mc + m
        x = F.relation_gather(P_logits, ctx, input)                                  # [B, feature + R C2, N]
        x = self.resize(x.reshape(bs, x.shape[1], *self.size))
        return {"x": x, "P_logits": P_logits}
