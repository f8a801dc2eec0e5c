"""CPU reference of the multi-style fast-style path: the conditional norm, the multi-style FastStyleNet and the
Dumoulin losses, composed from oracle/style_ref.py's pieces (stock torch, dtype-following: fp32 or fp64).

Restated (paths relative to the reference root):
  methods/learning-based/network.py:120-145   ConditionalBatchNorm2d
  methods/learning-based/network.py:147-298   ConvInstRelu / UpsampleConvInstRelu / FastStyleNet with n_styles > 1
                                              (the ResidualBlocks keep plain InstanceNorm2d(affine=True))
  methods/learning-based/fs_dumoulin.py:26-47 Dumoulin.train_method losses
tests/golden/multistyle_small.npz (tools/gen_golden_multistyle.py, produced by the reference's own modules) pins
it; tests/test_multistyle_host.py holds the two together.

Beyond the reference: a 1-D id tensor (one style per sample).  The reference's ``embed(y.long()).chunk(2)`` splits
dim 0, so it only takes a 0-dim id; the per-sample form here indexes the table row by row, which for N equal ids
is the same function of the inputs.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import style_ref

WIDTHS = {"conv1": 32, "conv2": 64, "conv3": 128, "deconv1": 64, "deconv2": 32}
COND_KEYS = tuple("%s.instance.%s" % (l, p) for l in WIDTHS for p in ("bn.weight", "bn.bias", "embed.weight"))


class RefCondNorm(nn.Module):
    def __init__(self, c, n_styles):
        super().__init__()
        self.num_features = c
        self.bn = nn.InstanceNorm2d(c, affine=True)
        self.embed = nn.Embedding(n_styles, 2 * c)
        with torch.no_grad():   # scale half N(1, 0.02), shift half 0
            self.embed.weight[:, c:].fill_(0.0)
            nn.init.normal_(self.embed.weight[:, :c], mean=1.0, std=0.02)

    def forward(self, x, y):
        out = self.bn(x)
        y = torch.as_tensor(y)
        c = self.num_features
        if y.dim() == 0:        # network.py:143-144: the row's two halves, broadcast over the batch
            gamma, beta = self.embed(y.long()).split(c)
        else:                   # one row per sample
            gamma, beta = self.embed(y.long()).split(c, dim=1)
        return gamma.reshape(-1, c, 1, 1) * out + beta.reshape(-1, c, 1, 1)


class RefCondConvInstRelu(style_ref.RefConvLayer):
    def __init__(self, cin, cout, k, stride, n_styles):
        super().__init__(cin, cout, k, stride)
        self.instance = RefCondNorm(cout, n_styles)

    def forward(self, x, y):
        return F.relu(self.instance(style_ref.RefConvLayer.forward(self, x), y))


class RefCondUpsampleConvInstRelu(nn.Module):
    def __init__(self, cin, cout, k, n_styles):
        super().__init__()
        self.reflection_pad = nn.ReflectionPad2d(k // 2)
        self.conv2d = nn.Conv2d(cin, cout, k, 1)
        self.instance = RefCondNorm(cout, n_styles)

    def forward(self, x, y):
        x = F.interpolate(x, scale_factor=2)
        return F.relu(self.instance(self.conv2d(self.reflection_pad(x)), y))


class RefMultiStyleNet(nn.Module):
    """network.py:263-298 FastStyleNet(num_inp, n_styles > 1); forward(x, style_strength, s_id) -> (features, image).
    s_id: int, 0-dim tensor (long / float, truncated by .long()) or a 1-D tensor / sequence of N ids."""

    def __init__(self, num_inp=3, n_styles=2):
        super().__init__()
        self.conv1 = RefCondConvInstRelu(num_inp, 32, 9, 1, n_styles)
        self.conv2 = RefCondConvInstRelu(32, 64, 3, 2, n_styles)
        self.conv3 = RefCondConvInstRelu(64, 128, 3, 2, n_styles)
        for i in range(1, 6):
            setattr(self, "res%d" % i, style_ref.RefResidualBlock(128))
        self.deconv1 = RefCondUpsampleConvInstRelu(128, 64, 3, n_styles)
        self.deconv2 = RefCondUpsampleConvInstRelu(64, 32, 3, n_styles)
        self.deconv3 = style_ref.RefConvLayer(32, 3, 9, 1)

    def forward(self, x, style_strength=1.0, s_id=0):
        s_id = torch.as_tensor(s_id)
        x = self.conv3(self.conv2(self.conv1(x, s_id), s_id), s_id)
        for i in range(1, 6):
            x = getattr(self, "res%d" % i)(x, style_strength)
        feats = x
        x = self.deconv3(self.deconv2(self.deconv1(x, s_id), s_id))
        return feats, torch.tanh(x / 255) * 150 + 255 / 2


def make(num_inp, n_styles, base, dtype=torch.float32):
    """RefMultiStyleNet with the counter-PRNG fixture weights style_ref.fsn_weights(net, base)."""
    net = RefMultiStyleNet(num_inp, n_styles)
    style_ref.load_np(net, style_ref.fsn_weights(net, base))
    return net.to(dtype)


def dumoulin_losses(model, vgg, img, styles, alpha, beta, style_id):
    """fs_dumoulin.py:26-47 train_method: styles[style_id] = that style's Grams per level.
    Returns (loss, content, style, styled / 255)."""
    _, styled = model(img, s_id=style_id)
    styled = styled / 255.0
    sf = vgg(style_ref.normalize(styled))
    imf = vgg(style_ref.normalize(img))
    content = alpha * F.mse_loss(sf[2], imf[2])
    style = 0
    for i, gs in enumerate(styles[int(style_id)]):
        style = style + ((style_ref.gram_matrix(sf[i]) - gs) ** 2).mean()
    style = style * beta
    return content + style, content, style, styled
