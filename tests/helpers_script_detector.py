"""A synthetic stand-in for the detector side of NVIDIA's TorchScript `vgg16.pt`: VGG16 topology at reduced width with its fifth pool
and three fully connected layers, random weights, the call signature the reference uses
(`module(x, return_features=True)`, metrics/metric_utils.py:318, and `module(x, resize_images=False, return_lpips=True)`), an
ImageNet-style input layer held in buffers and the five LPIPS channel weights as [1,C,1,1] buffers.  The module resizes its input to
S x S itself, by 'area' or 'bilinear', and returns the activation after fc1 + ReLU, after fc2 + ReLU, or -- a layout no loader
candidate covers -- the raw logits of fc3.  Scripted with torch.jit.script and saved, so that loading goes through torch.jit.load.
Test data only -- no reference source is involved."""
import torch
import torch.nn as nn
import torch.nn.functional as F

_CFG = [(1, 2), (2, 2), (4, 3), (8, 3), (8, 3)]


class _ScriptDetectorVGG(nn.Module):
    def __init__(self, width=8, size=32, seed=5, resize='area', features_after=2, fc_widths=(40, 24, 10)):
        super().__init__()
        assert resize in ('area', 'bilinear') and features_after in (1, 2, 3) and size % 32 == 0
        g = torch.Generator().manual_seed(seed)
        convs, c, chans = [], 3, []
        for mult, n in _CFG:
            for _ in range(n):
                co = mult * width
                m = nn.Conv2d(c, co, 3, padding=1)
                with torch.no_grad():
                    m.weight.copy_(torch.randn([co, c, 3, 3], generator=g) * (2.0 / (c * 9)) ** 0.5)
                    m.bias.copy_(torch.randn([co], generator=g) * 0.05 + 0.05)
                convs.append(m)
                c = co
            chans.append(c)
        self.layers = nn.ModuleList(convs)
        for i, ch in enumerate(chans):
            self.register_buffer(f'lpips{i}', torch.rand([1, ch, 1, 1], generator=g) + 0.1)
        self.register_buffer('mean', torch.tensor([123.675, 116.28, 103.53]).reshape(1, 3, 1, 1))
        self.register_buffer('std', torch.tensor([58.395, 57.12, 57.375]).reshape(1, 3, 1, 1))
        k = c * (size // 32) ** 2
        fcs = []
        for o in fc_widths:
            m = nn.Linear(k, o)
            with torch.no_grad():
                m.weight.copy_(torch.randn([o, k], generator=g) * (2.0 / k) ** 0.5)
                m.bias.copy_(torch.randn([o], generator=g) * 0.1 + 0.1)
            fcs.append(m)
            k = o
        self.fc1, self.fc2, self.fc3 = fcs
        self.size = size
        self.area = resize == 'area'
        self.features_after = features_after

    def _pack(self, f, lin):
        n = f * torch.rsqrt(f.square().sum(dim=1, keepdim=True) + 1e-10)
        return (n * lin.sqrt() / float(f.shape[2] * f.shape[3]) ** 0.5).flatten(1)

    def forward(self, img, resize_images: bool = True, return_features: bool = False, return_lpips: bool = False):
        x = img.to(torch.float32)
        if resize_images and (x.shape[2] != self.size or x.shape[3] != self.size):
            if self.area:
                x = F.interpolate(x, size=(self.size, self.size), mode='area')
            else:
                x = F.interpolate(x, size=(self.size, self.size), mode='bilinear', align_corners=False)
        x = (x - self.mean) / self.std
        outs = []
        k = 0
        for conv in self.layers:
            x = F.relu(conv(x))
            if k == 1:
                outs.append(self._pack(x, self.lpips0))
                x = F.max_pool2d(x, 2)
            elif k == 3:
                outs.append(self._pack(x, self.lpips1))
                x = F.max_pool2d(x, 2)
            elif k == 6:
                outs.append(self._pack(x, self.lpips2))
                x = F.max_pool2d(x, 2)
            elif k == 9:
                outs.append(self._pack(x, self.lpips3))
                x = F.max_pool2d(x, 2)
            elif k == 12:
                outs.append(self._pack(x, self.lpips4))
            k += 1
        if return_lpips:
            return torch.cat(outs, dim=1)
        x = F.max_pool2d(x, 2).flatten(1)
        x = F.relu(self.fc1(x))
        if return_features and self.features_after == 1:
            return x
        x = F.relu(self.fc2(x))
        if return_features and self.features_after == 2:
            return x
        x = self.fc3(x)
        if return_features:
            return x
        return torch.softmax(x, dim=1)


def save_scripted_detector(path, **kw):
    m = torch.jit.script(_ScriptDetectorVGG(**kw).eval())
    m.save(str(path))
    return m


def reference_side_features(module, images):
    """what the reference computes for a batch in [-1, 1] (metric_utils.py:314-318): repeat, torch's own quantisation, the scripted
    module on the host"""
    x = images.detach().cpu()
    if x.shape[1] == 1:
        x = x.repeat([1, 3, 1, 1])
    x = (x * 127.5 + 128).clamp(0, 255).to(torch.uint8)
    with torch.no_grad():
        return module(x, return_features=True).to(torch.float32)
