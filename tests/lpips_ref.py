"""fp64 restatement of LPIPS (AlexNet), written from the published definition of the lpips 0.1.x package (scaling layer,
torchvision's AlexNet feature stack with a tap after each of the five ReLUs, unit-normalised channel vectors with the
epsilon outside the root, 1x1 "lin" weights, spatial mean, sum over the taps; no 2x - 1 rescale: the reference calls it
with normalize=False) in plain torch CPU ops.  Not the package itself, which the test machines do not have, and no
pretrained weights: every test runs on seeded random ones."""
import torch
import torch.nn.functional as F

# (C_out, C_in, k, stride, pad) of the five convolutions; a 3x3 stride-2 floor-mode max pool precedes conv1 and conv2
LAYERS = ((64, 3, 11, 4, 2), (192, 64, 5, 1, 2), (384, 192, 3, 1, 1), (256, 384, 3, 1, 1), (256, 256, 3, 1, 1))
POOL_BEFORE = (False, True, True, False, False)
# fp32 buffers in the package, so the fp32-rounded values are the definition
SHIFT = torch.tensor([-.030, -.088, -.188], dtype=torch.float32).double()
SCALE = torch.tensor([.458, .448, .450], dtype=torch.float32).double()


def random_weights(seed):
    """{"convs": [(W, b)] * 5, "lins": [w] * 5}: He-scaled convolution weights, biases 0.1 * randn, lin weights rand(C), rounded
    to fp32 once so that both sides see the same numbers."""
    g = torch.Generator().manual_seed(seed)
    convs, lins = [], []
    for co, ci, k, _, _ in LAYERS:
        w = torch.randn(co, ci, k, k, generator=g, dtype=torch.float64) * (2.0 / (ci * k * k)) ** 0.5
        b = 0.1 * torch.randn(co, generator=g, dtype=torch.float64)
        convs.append((w.float(), b.float()))
        lins.append(torch.rand(co, generator=g, dtype=torch.float64).float())
    return {"convs": convs, "lins": lins}


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def layer_input_sizes(H, W):
    """The (H, W) each of the five convolutions sees for an H x W image."""
    sizes, h, w = [], H, W
    for (_, _, k, s, p), pool in zip(LAYERS, POOL_BEFORE):
        if pool:
            h, w = out_size(h, 3, 2, 0), out_size(w, 3, 2, 0)
        sizes.append((h, w))
        h, w = out_size(h, k, s, p), out_size(w, k, s, p)
    return sizes


def scale_input(x):
    return (x.double() - SHIFT[None, :, None, None]) / SCALE[None, :, None, None]


def conv(x, W, b, layer, relu=True):
    """One convolution in fp64 (zero padding of x as given)."""
    _, _, _, s, p = LAYERS[layer]
    y = F.conv2d(x.double(), W.double(), b.double(), stride=s, padding=p)
    return F.relu(y) if relu else y


def abs_bound(x, W, b, layer):
    """conv(|x|, |W|) + |b| in fp64: what the rounding error of a fp32 sum of these terms is relative to."""
    _, _, _, s, p = LAYERS[layer]
    return F.conv2d(x.double().abs(), W.double().abs(), b.double().abs(), stride=s, padding=p)


def features(x, w):
    """The five taps of (N, 3, H, W) images, fp64."""
    h = scale_input(x)
    taps = []
    for i, (W, b) in enumerate(w["convs"]):
        if POOL_BEFORE[i]:
            h = F.max_pool2d(h, 3, 2)
        h = conv(h, W, b, i)
        taps.append(h)
    return taps


def lpips(a, b, w, dtype=torch.float64):
    """LPIPS of (N, 3, H, W) images a against b, one value per pair; dtype=torch.float32 runs the same computation in fp32
    (what the fp64 reference's own distance from a careful fp32 evaluation is measured with)."""
    if dtype == torch.float64:
        fa, fb = features(a, w), features(b, w)
    else:
        def feats(x):
            h = ((x - SHIFT.float()[None, :, None, None]) / SCALE.float()[None, :, None, None])
            taps = []
            for i, (W, bb) in enumerate(w["convs"]):
                if POOL_BEFORE[i]:
                    h = F.max_pool2d(h, 3, 2)
                _, _, _, s, p = LAYERS[i]
                h = F.relu(F.conv2d(h, W, bb, stride=s, padding=p))
                taps.append(h)
            return taps
        fa, fb = feats(a.float()), feats(b.float())
    total = 0
    for x, y, lin in zip(fa, fb, w["lins"]):
        xn = x / (x.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        yn = y / (y.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        total = total + ((xn - yn) ** 2 * lin.to(x.dtype)[None, :, None, None]).sum(1).flatten(1).mean(1)
    return total.double()
