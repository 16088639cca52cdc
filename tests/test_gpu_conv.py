"""GPU parity of the conv autoencoder forward against the reference's goldens and the
oracle (fp64), incl. the <=1e-5 decoder-pixel target of BASELINE.json."""
import pytest
import torch

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

PIX_TOL = 1e-5  # max|err| / max|ref| on decoder pixels (north_star)


@pytest.mark.parametrize("N,Cin,H,W,Cout,stride,act", [
    (2, 3, 16, 16, 8, 1, 1), (1, 16, 9, 13, 20, 1, 0), (2, 8, 16, 16, 16, 2, 1),
    (1, 32, 8, 8, 3, 1, 2), (2, 130, 12, 10, 140, 1, 1), (1, 4, 7, 7, 4, 2, 3)])
def test_conv2d_fwd(N, Cin, H, W, Cout, stride, act):
    from qarig import ops
    from oracle import ref_models as rm
    g = torch.Generator().manual_seed(Cin + Cout)
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, 3, 3), generator=g) / (3 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    y, pre = ops.conv2d_fwd(x.cuda(), w.cuda(), b.cuda(), stride, 1, act, want_preact=True)
    ref = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=1)
    assert rel_err(pre, ref) < 2e-6
    assert rel_err(y, rm.activation(ref, {0: None, 1: "silu", 2: "tanh", 3: "sigmoid"}[act])) < 4e-6


@pytest.mark.parametrize("N,Cin,H,W,Cout", [(2, 8, 4, 4, 8), (1, 20, 5, 7, 12), (1, 64, 8, 8, 3),
                                            (2, 16, 6, 6, 140)])
def test_conv_transpose2d_fwd(N, Cin, H, W, Cout):
    from qarig import ops
    g = torch.Generator().manual_seed(Cin * Cout)
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cin, Cout, 4, 4), generator=g) / (4 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    y = ops.conv_transpose2d_fwd(x.cuda(), w.cuda(), b.cuda(), 1)
    ref = torch.nn.functional.silu(torch.nn.functional.conv_transpose2d(
        x.double(), w.double(), b.double(), stride=2, padding=1))
    assert y.shape == ref.shape
    assert rel_err(y, ref) < 4e-6


def test_autoencoder_vs_reference_golden():
    from models.Autoencoder import Autoencoder
    from models.FC_Decoder import FC_Decoder
    from models.FC_Encoder import FC_Encoder
    g = load_golden("autoencoder")
    m = Autoencoder(num_layers=2, image_channel=3, min_channel=8, max_channel=16, latent_channel=4,
                    encoder_activation_type="tanh")
    m.custom_load_state_dict(g["sd"])
    m = m.cuda()
    with torch.no_grad():
        z = m.get_latent(g["x"].cuda())
        y = m.recon_image(z)
        y2 = m(g["x"].cuda())
    assert rel_err(z, g["latent"]) < PIX_TOL
    assert rel_err(y, g["recon"]) < PIX_TOL and torch.equal(y, y2)
    # bare halves through the loader hacks (prefix rewrite, "decoder" filter)
    enc = FC_Encoder(num_layers=2, image_channel=3, min_channel=8, max_channel=16, latent_channel=4)
    enc.custom_load_state_dict(g["sd"], ignore_msgs=True)
    dec = FC_Decoder(num_layers=2, image_channel=3, min_channel=8, max_channel=16, latent_channel=4)
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        dec.custom_load_state_dict(g["sd"])
    with torch.no_grad():
        assert torch.equal(enc.cuda()(g["x"].cuda()), z)
        assert torch.equal(dec.cuda()(z), y)


def test_decoder_wide_vs_reference_golden():
    from models.FC_Decoder import FC_Decoder
    g = load_golden("decoder_wide")
    dec = FC_Decoder(num_layers=2, image_channel=3, min_channel=32, max_channel=64, latent_channel=4)
    dec.custom_load_state_dict(g["sd"])
    with torch.no_grad():
        y = dec.cuda()(g["z"].cuda())
    assert rel_err(y, g["recon"]) < PIX_TOL


def test_decoder_readme_shape_pixels_vs_oracle_fp64():
    """README decoder (256/512 channels, 32x32x4 latent -> 128x128x3), default init:
    pixel rel-err vs the oracle evaluated in fp64 must meet the 1e-5 target."""
    from models.FC_Decoder import FC_Decoder
    from oracle import ref_models as rm
    torch.manual_seed(3)
    dec = FC_Decoder(num_layers=2, image_channel=3, min_channel=256, max_channel=512,
                     latent_channel=4)
    z = torch.tanh(torch.randn((1, 4, 32, 32), generator=torch.Generator().manual_seed(1)))
    sd64 = {k: v.double() for k, v in dec.state_dict().items()}
    ref = rm.fc_decoder(sd64, z.double())
    with torch.no_grad():
        y = dec.cuda()(z.cuda())
    assert y.shape == (1, 3, 128, 128)
    assert rel_err(y, ref) < PIX_TOL


@pytest.mark.parametrize("N,Cin,H,W,Cout,stride,act", [
    (2, 3, 16, 16, 8, 1, 1), (1, 16, 9, 13, 20, 1, 0), (2, 8, 16, 16, 16, 2, 1),
    (1, 32, 8, 8, 3, 1, 2), (2, 130, 12, 10, 140, 1, 1), (1, 4, 7, 9, 12, 2, 3),
    (1, 3, 32, 32, 64, 1, 1)])      # input gradient to 3 channels: the direct kernel's channel-split form, flipped taps
def test_conv2d_bwd(N, Cin, H, W, Cout, stride, act):
    from conftest import grad_err
    from qarig import functional as QF
    from oracle import ref_models as rm
    g = torch.Generator().manual_seed(Cin + Cout + 1)
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, 3, 3), generator=g) / (3 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    name = {0: None, 1: "silu", 2: "tanh", 3: "sigmoid"}[act]
    a = [t.double().requires_grad_(True) for t in (x, w, b)]
    ya = rm.activation(torch.nn.functional.conv2d(a[0], a[1], a[2], stride=stride, padding=1), name)
    dy = torch.randn(ya.shape, generator=g)
    (ya * dy.double()).sum().backward()
    c = [t.cuda().requires_grad_(True) for t in (x, w, b)]
    yc = QF.conv2d_act(c[0], c[1], c[2], stride, 1, act)
    (yc * dy.cuda()).sum().backward()
    for p, q in zip(c, a):
        assert grad_err(p.grad, q.grad) < 1e-5


@pytest.mark.parametrize("N,Cin,H,W,Cout", [(2, 8, 4, 4, 8), (1, 20, 5, 7, 12), (1, 64, 8, 8, 3),
                                            (2, 16, 6, 6, 140)])
def test_conv_transpose2d_bwd(N, Cin, H, W, Cout):
    from conftest import grad_err
    from qarig import functional as QF
    g = torch.Generator().manual_seed(Cin * Cout + 1)
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cin, Cout, 4, 4), generator=g) / (4 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    a = [t.double().requires_grad_(True) for t in (x, w, b)]
    ya = torch.nn.functional.silu(torch.nn.functional.conv_transpose2d(a[0], a[1], a[2], stride=2,
                                                                       padding=1))
    dy = torch.randn(ya.shape, generator=g)
    (ya * dy.double()).sum().backward()
    c = [t.cuda().requires_grad_(True) for t in (x, w, b)]
    yc = QF.conv_transpose2d_act(c[0], c[1], c[2], 1)
    (yc * dy.cuda()).sum().backward()
    for p, q in zip(c, a):
        assert grad_err(p.grad, q.grad) < 1e-5


def test_autoencoder_train_grads_vs_reference_golden():
    """BASELINE config 1 shape family (tiny): MSE recon loss, every parameter gradient
    and the input gradient against what the reference's autograd produced."""
    from conftest import grad_err
    from models.Autoencoder import Autoencoder
    g = load_golden("autoencoder")
    m = Autoencoder(num_layers=2, image_channel=3, min_channel=8, max_channel=16, latent_channel=4,
                    encoder_activation_type="tanh")
    m.custom_load_state_dict(g["sd"])
    m = m.cuda()
    x = g["x"].cuda().requires_grad_(True)
    y = m(x)
    loss = ((y - x.detach()) ** 2).mean()
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-6
    assert grad_err(x.grad, g["x_grad"]) < 2e-5
    for n, p in m.named_parameters():
        assert grad_err(p.grad, g["grads"][n]) < 2e-5, n


# ---- interior ("FAST") kernels at README channel counts ---------------------------------------
# conv.hip takes its branch-free interior kernels only when the channel counts are multiples
# of 128 (forward: Cout % 128, weight gradient: Cg % 128, pixels % 128); the small shapes above
# never reach them.  N=2 at 32x32 (1024 pixels per image) does, for every layer type of the
# README autoencoder (256/512 channels): forward, d-input, d-weight, d-bias vs fp64.
@pytest.mark.parametrize("Cin,Cout,stride", [(256, 256, 1), (256, 512, 2), (512, 512, 1), (512, 512, 2)])
def test_conv2d_readme_channels_fwd_bwd_vs_fp64(Cin, Cout, stride):
    from conftest import grad_err
    from qarig import functional as QF
    g = torch.Generator().manual_seed(Cin + Cout + stride)
    N, H, W = 2, 32, 32
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, 3, 3), generator=g) / (3 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    a = [t.double().requires_grad_(True) for t in (x, w, b)]
    ya = torch.nn.functional.silu(torch.nn.functional.conv2d(a[0], a[1], a[2], stride=stride, padding=1))
    dy = torch.randn(ya.shape, generator=g)
    (ya * dy.double()).sum().backward()
    c = [t.cuda().requires_grad_(True) for t in (x, w, b)]
    yc = QF.conv2d_act(c[0], c[1], c[2], stride, 1, 1)
    assert rel_err(yc, ya) < 4e-6
    (yc * dy.cuda()).sum().backward()
    for p, q in zip(c, a):
        assert grad_err(p.grad, q.grad) < 1e-5


@pytest.mark.parametrize("Cin,Cout", [(512, 256), (256, 256)])
def test_conv_transpose2d_readme_channels_fwd_bwd_vs_fp64(Cin, Cout):
    from conftest import grad_err
    from qarig import functional as QF
    g = torch.Generator().manual_seed(Cin * 3 + Cout)
    N, H, W = 2, 16, 16
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cin, Cout, 4, 4), generator=g) / (4 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    a = [t.double().requires_grad_(True) for t in (x, w, b)]
    ya = torch.nn.functional.silu(torch.nn.functional.conv_transpose2d(a[0], a[1], a[2], stride=2, padding=1))
    dy = torch.randn(ya.shape, generator=g)
    (ya * dy.double()).sum().backward()
    c = [t.cuda().requires_grad_(True) for t in (x, w, b)]
    yc = QF.conv_transpose2d_act(c[0], c[1], c[2], 1)
    assert rel_err(yc, ya) < 4e-6
    (yc * dy.cuda()).sum().backward()
    for p, q in zip(c, a):
        assert grad_err(p.grad, q.grad) < 1e-5


def test_encoder_readme_shape_latent_vs_oracle_fp64():
    """README encoder (256/512 channels, 2 down levels, 3x64x64 -> 4x16x16), default init: latent
    rel-err vs the oracle in fp64 (the stride-2 and 512-channel interior kernels)."""
    from models.FC_Encoder import FC_Encoder
    from oracle import ref_models as rm
    torch.manual_seed(5)
    enc = FC_Encoder(num_layers=2, image_channel=3, min_channel=256, max_channel=512, latent_channel=4,
                     use_final_activation=True, final_activation_type="tanh")
    x = 2 * torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(0)) - 1
    sd64 = {k: v.double() for k, v in enc.state_dict().items()}
    ref = rm.fc_encoder(sd64, x.double(), final_act="tanh")
    with torch.no_grad():
        z = enc.cuda()(x.cuda())
    assert z.shape == (2, 4, 16, 16)
    assert rel_err(z, ref) < PIX_TOL


def test_config0_autoencoder_train_step_vs_oracle_fp64():
    """BASELINE configs[0] as a step: README autoencoder (256 / 512 channels, 2 levels, latent 4), batch 4 of
    64 x 64 x 3, reconstruction MSE + backward + Adam(0.5, 0.999) (reference train_autoencoder.py:203-226) --
    loss, EVERY parameter gradient and the post-Adam weights against the oracle evaluated in fp64."""
    from conftest import grad_err
    from models.Autoencoder import Autoencoder
    from oracle import ref_models as rm
    from qarig import functional as QF
    from qarig.optim import FlatAdam
    torch.manual_seed(3)
    m = Autoencoder(num_layers=2, image_channel=3, min_channel=256, max_channel=512, latent_channel=4)
    x = torch.rand((4, 3, 64, 64), generator=torch.Generator().manual_seed(0)) * 2 - 1
    sd = {k: v.detach().double().requires_grad_(True) for k, v in m.state_dict().items()}
    names = list(sd)
    recon = rm.autoencoder(sd, x.double())
    ref_loss = torch.mean((recon - x.double()) ** 2)
    ref_grads = torch.autograd.grad(ref_loss, [sd[k] for k in names])
    before = {k: v.detach().clone() for k, v in sd.items()}
    lr = 1e-4
    with torch.no_grad():
        rm.adam_step([sd[k] for k in names], ref_grads, [torch.zeros_like(sd[k]) for k in names],
                     [torch.zeros_like(sd[k]) for k in names], 1, lr)
    m = m.cuda()
    opt = FlatAdam(m.parameters(), lr=lr, betas=(0.5, 0.999))
    opt.zero_grad()
    xg = x.cuda()
    out = m(xg)
    assert rel_err(out, recon) < PIX_TOL
    loss = QF.mse_loss(out, xg)
    loss.backward()
    assert abs(float(loss) - float(ref_loss)) < 1e-5 * max(1.0, abs(float(ref_loss)))
    got = dict(m.named_parameters())
    assert set(got) == set(names)
    for k, g in zip(names, ref_grads):
        assert grad_err(got[k].grad, g) < 2e-5, k
    opt.step()
    for k, g in zip(names, ref_grads):
        w = got[k].detach().double().cpu()
        # first Adam step: the update is lr * g / (|g| + eps), i.e. +-lr wherever the gradient is not noise;
        # compared where the fp64 gradient is well above the 2e-5 gradient tolerance, bounded by 2 lr elsewhere
        # (a component inside the tolerance may legitimately take the other sign)
        clear = g.abs() > 1e-3 * g.abs().max()
        d = (w - sd[k].detach()).abs()
        assert float(d[clear].max()) <= 2e-3 * lr + 1e-7 * float(before[k].abs().max()), k
        assert float(d.max()) <= 2.0 * lr + 1e-7, k


def test_conv_autograd_node_accepts_non_contiguous_input():
    """The autograd node normalises its input once and saves THAT tensor: a channels-last view
    must give the gradients of the dense tensor."""
    from qarig import functional as QF
    g = torch.Generator().manual_seed(9)
    x = torch.randn((2, 8, 10, 12), generator=g).cuda()
    w = (torch.randn((16, 8, 3, 3), generator=g) / 8).cuda().requires_grad_(True)
    b = torch.randn(16, generator=g).cuda().requires_grad_(True)
    dy = torch.randn((2, 16, 10, 12), generator=g).cuda()
    res = []
    for xin in (x, x.to(memory_format=torch.channels_last)):
        xin = xin.detach().requires_grad_(True)
        w.grad = b.grad = None
        (QF.conv2d_act(xin, w, b, 1, 1, 1) * dy).sum().backward()
        res.append((xin.grad.contiguous().clone(), w.grad.clone(), b.grad.clone()))
    for a, c in zip(*res):
        assert torch.equal(a, c)


@pytest.mark.parametrize("N,Cin,H,W,Cout,act", [
    (8, 16, 4, 4, 128, 0),        # every group is both first and last of its row; a pixel tile spans 8 images
    (2, 32, 8, 8, 128, 1),        # two groups per row
    (1, 48, 16, 24, 256, 2),      # W not a power of two
    (2, 256, 32, 32, 256, 1),     # README residual block
    (3, 16, 128, 4, 128, 3),      # tall, 4 wide
    (2, 128, 8, 8, 48, 1),        # forward on the gather kernel, input gradient (128 x 48) on the ring
    (2, 128, 16, 16, 128, 0),     # weight gradient on the ring too: one k-tile per image row (every tile meets the border)
    (1, 128, 8, 48, 128, 1),      # three k-tiles per row
    (3, 128, 16, 32, 256, 1),     # pixel splits that do not divide evenly
])
def test_conv3x3_ring_kernel_fwd_bwd_vs_fp64(N, Cin, H, W, Cout, act):
    """The 3x3 / stride 1 / padding 1 layers whose tiles are whole run on csrc/conv.hip
    conv3x3_ring_kernel (tap-major reduction, weights by LDS-DMA, im2col by range-checked buffer loads with
    the image border handled by selects): forward, input gradient (the same kernel on flipped weights when
    Cout % 16 == 0 and Cin % 128 == 0) and weight gradient against fp64, at the tolerances of the other
    conv tests."""
    from conftest import grad_err
    from qarig import functional as QF
    from oracle import ref_models as rm
    g = torch.Generator().manual_seed(N + Cin + H + W + Cout)
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, 3, 3), generator=g) / (3 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    name = {0: None, 1: "silu", 2: "tanh", 3: "sigmoid"}[act]
    a = [t.double().requires_grad_(True) for t in (x, w, b)]
    ya = rm.activation(torch.nn.functional.conv2d(a[0], a[1], a[2], stride=1, padding=1), name)
    dy = torch.randn(ya.shape, generator=g)
    (ya * dy.double()).sum().backward()
    c = [t.cuda().requires_grad_(True) for t in (x, w, b)]
    yc = QF.conv2d_act(c[0], c[1], c[2], 1, 1, act)
    assert rel_err(yc, ya) < 4e-6
    (yc * dy.cuda()).sum().backward()
    for p, q in zip(c, a):
        assert grad_err(p.grad, q.grad) < 1e-5
    # deterministic
    assert torch.equal(QF.conv2d_act(c[0], c[1], c[2], 1, 1, act), yc)


@pytest.mark.parametrize("N,Cin,H,W,Cout", [(8, 16, 4, 4, 128), (2, 32, 8, 8, 128), (1, 48, 16, 24, 256),
                                            (3, 64, 32, 4, 128)])
def test_conv_transpose2d_ring_kernel_vs_fp64(N, Cin, H, W, Cout):
    """ConvTranspose2d(4, 2, 1) forward as four 2x2-tap stride-1 products on the ring kernel (two column
    parities per workgroup, 8-B stores): narrow images (every pixel group touches a border), tiles spanning
    images, channel counts that leave a remainder of ring bodies; saved pre-activation included."""
    from qarig import ops
    g = torch.Generator().manual_seed(N * 7 + Cin + H + W + Cout)
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cin, Cout, 4, 4), generator=g) / (4 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    ref = torch.nn.functional.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1)
    y, pre = ops.conv_transpose2d_fwd(x.cuda(), w.cuda(), b.cuda(), 1, want_preact=True)
    assert y.shape == ref.shape
    assert rel_err(pre, ref) < 2e-6
    assert rel_err(y, torch.nn.functional.silu(ref)) < 4e-6
    assert torch.equal(ops.conv_transpose2d_fwd(x.cuda(), w.cuda(), b.cuda(), 1), y)


@pytest.mark.parametrize("N,Cin,H,W,Cout", [(2, 128, 16, 16, 32), (8, 128, 8, 8, 16), (1, 256, 32, 48, 48),
                                            (2, 256, 32, 32, 512)])
def test_conv2d_stride2_input_gradient_ring_vs_fp64(N, Cin, H, W, Cout):
    """Input gradient of Conv2d(3, stride 2, padding 1) as four parity classes of 1 / 2 / 2 / 4 taps on the ring
    kernel (csrc/conv.hip conv3x3_ring_kernel<PAIR>, mode 1), with every gradient of the layer against fp64."""
    from conftest import grad_err
    from qarig import functional as QF
    g = torch.Generator().manual_seed(N + Cin + H + W + Cout + 2)
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, 3, 3), generator=g) / (3 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    a = [t.double().requires_grad_(True) for t in (x, w, b)]
    ya = torch.nn.functional.silu(torch.nn.functional.conv2d(a[0], a[1], a[2], stride=2, padding=1))
    dy = torch.randn(ya.shape, generator=g)
    (ya * dy.double()).sum().backward()
    c = [t.cuda().requires_grad_(True) for t in (x, w, b)]
    yc = QF.conv2d_act(c[0], c[1], c[2], 2, 1, 1)
    assert rel_err(yc, ya) < 4e-6
    (yc * dy.cuda()).sum().backward()
    for p, q in zip(c, a):
        assert grad_err(p.grad, q.grad) < 1e-5


@pytest.mark.parametrize("N,Cin,H,W,Cout,act", [(8, 16, 8, 8, 128, 0), (2, 32, 16, 16, 128, 1), (1, 48, 32, 48, 256, 2),
                                                (2, 256, 64, 64, 512, 1)])
def test_conv2d_stride2_forward_ring_vs_fp64(N, Cin, H, W, Cout, act):
    """Conv2d(3, stride 2, padding 1) forward on the ring kernel with the strided im2col (four 4-B buffer
    loads per k row; only the top row / left column of the padding can be touched): output and saved
    pre-activation against fp64, narrow and non-power-of-two widths, tiles spanning images."""
    from qarig import ops
    from oracle import ref_models as rm
    g = torch.Generator().manual_seed(N + Cin + H + W + Cout + 11)
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, 3, 3), generator=g) / (3 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    y, pre = ops.conv2d_fwd(x.cuda(), w.cuda(), b.cuda(), 2, 1, act, want_preact=True)
    ref = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1)
    assert rel_err(pre, ref) < 2e-6
    assert rel_err(y, rm.activation(ref, {0: None, 1: "silu", 2: "tanh", 3: "sigmoid"}[act])) < 4e-6
    assert torch.equal(ops.conv2d_fwd(x.cuda(), w.cuda(), b.cuda(), 2, 1, act), y)


@pytest.mark.parametrize("N,Cin,H,W,Cout", [(8, 128, 4, 4, 16), (1, 128, 16, 24, 48), (2, 256, 8, 8, 32)])
def test_conv_transpose2d_input_gradient_ring_vs_fp64(N, Cin, H, W, Cout):
    """Input gradient of ConvTranspose2d(4, 2, 1) = Conv2d(4, stride 2, padding 1) over dT: 16 taps at offsets
    -1 .. 2 on the strided ring kernel (rows / columns past the far edge included), all gradients vs fp64."""
    from conftest import grad_err
    from qarig import functional as QF
    g = torch.Generator().manual_seed(N + Cin * 3 + H + W + Cout)
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cin, Cout, 4, 4), generator=g) / (4 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    a = [t.double().requires_grad_(True) for t in (x, w, b)]
    ya = torch.nn.functional.silu(torch.nn.functional.conv_transpose2d(a[0], a[1], a[2], stride=2, padding=1))
    dy = torch.randn(ya.shape, generator=g)
    (ya * dy.double()).sum().backward()
    c = [t.cuda().requires_grad_(True) for t in (x, w, b)]
    yc = QF.conv_transpose2d_act(c[0], c[1], c[2], 1)
    assert rel_err(yc, ya) < 4e-6
    (yc * dy.cuda()).sum().backward()
    for p, q in zip(c, a):
        assert grad_err(p.grad, q.grad) < 1e-5


@pytest.mark.parametrize("kind,N,Cin,H,W,Cout", [
    ("conv", 1, 64, 16, 16, 128),       # 2 tiles, 36 k-tiles: 2 parts
    ("conv", 4, 256, 32, 32, 128),      # 32 tiles: 8 parts of 18 k-tiles, parts start inside a tap
    ("conv", 2, 512, 16, 16, 256),      # 8 tiles: 8 parts of 36
    ("convt", 4, 256, 16, 16, 128),     # 16 workgroups x 2 column parities, 4 parts of 16 k-tiles
    ("convt", 1, 512, 32, 32, 256),     # the README upsampling layer at one image: 8 parts
    ("direct", 4, 256, 64, 64, 3),      # the decoder's last layer: channels split over 8 waves
    ("direct", 1, 64, 16, 16, 4),
    ("s2", 2, 128, 32, 32, 256),        # the other ring products fall back through the same code (run_conv_ring):
    ("dgrad", 1, 128, 16, 16, 128),     # stride-2 forward, 3x3 input gradient, ConvTranspose input gradient
    ("convt_dgrad", 2, 128, 16, 16, 128)])
def test_few_image_launches_split_the_reduction(kind, N, Cin, H, W, Cout):
    """At few images (generate_images.py:366 decodes the handful just sampled) the ring launches have too
    few tiles to fill the chip: the reduction is split over blockIdx.z into slabs that
    conv_split_reduce_kernel adds in order (+ bias, activation, saved pre-activation); the <= 4-channel
    output layer splits its channels over the waves of a workgroup.  Against fp64, and against the
    unsplit launch (a workspace without room for the slabs), which it must match to rounding but not
    bit for bit (proof that the split form ran)."""
    from qarig import ops, _lib
    from qarig._lib import ptr
    lib = _lib.load()
    g = torch.Generator().manual_seed(N * 3 + Cin + Cout)
    x = torch.randn((N, Cin, H, W), generator=g)
    b = torch.randn(Cout, generator=g)
    if kind in ("s2", "dgrad", "convt_dgrad"):
        # the entry point itself, once with the scratch its _n function asks for and once with the packed weights' only
        F = torch.nn.functional
        if kind == "s2":
            w = torch.randn((Cout, Cin, 3, 3), generator=g) / (3 * Cin ** 0.5)
            ref = F.silu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1))
            small, big = (lib.qarig_conv2d_fwd_workspace_bytes(Cin, Cout, 3),
                          lib.qarig_conv2d_fwd_workspace_bytes_n(N, Cin, H, W, Cout, 3, 2))
            src, bc = x.cuda(), b.cuda()
            call = lambda out, ws, n: lib.qarig_conv2d_fwd_ws(ptr(src), N, Cin, H, W, ptr(wc), ptr(bc), Cout, 3, 2, 1, 1,
                                                              ptr(out), None, ptr(ws), n, 0, _lib.stream())
        elif kind == "dgrad":
            w = torch.randn((Cout, Cin, 3, 3), generator=g) / (3 * Cin ** 0.5)
            dT = torch.randn((N, Cout, H, W), generator=g)
            ref = F.conv_transpose2d(dT.double(), w.double(), stride=1, padding=1)
            small, big = (lib.qarig_conv2d_bwd_data_workspace_bytes(Cin, Cout, 3),
                          lib.qarig_conv2d_bwd_data_workspace_bytes_n(N, Cin, H, W, Cout, 3, 1))
            src = dT.cuda()
            call = lambda out, ws, n: lib.qarig_conv2d_bwd_data(ptr(src), N, Cout, H, W, ptr(wc), Cin, 3, 1, 1, H, W,
                                                                ptr(out), ptr(ws), n, _lib.stream())
        else:
            w = torch.randn((Cin, Cout, 4, 4), generator=g) / (4 * Cin ** 0.5)
            dT = torch.randn((N, Cout, 2 * H, 2 * W), generator=g)
            ref = F.conv2d(dT.double(), w.double(), stride=2, padding=1)
            small, big = (lib.qarig_conv_transpose2d_workspace_bytes(Cin, Cout),
                          lib.qarig_conv_transpose2d_bwd_data_workspace_bytes_n(N, Cin, H, W, Cout))
            src = dT.cuda()
            call = lambda out, ws, n: lib.qarig_conv_transpose2d_bwd_data_ws(ptr(src), N, Cout, H, W, ptr(wc), Cin,
                                                                             ptr(out), ptr(ws), n, _lib.stream())
        assert big > small
        wc = w.cuda()
        ws = torch.empty(big, dtype=torch.uint8, device="cuda")
        y, y1 = (torch.empty(ref.shape, dtype=torch.float32, device="cuda") for _ in range(2))
        rc, rc1 = call(y, ws, big), call(y1, ws, small)
        torch.cuda.synchronize()
        assert rc == 0 and rc1 == 0
        assert rel_err(y, ref) < 4e-6
        assert rel_err(y1, y) < 5e-6 and not torch.equal(y1, y)
        return
    if kind == "convt":
        w = torch.randn((Cin, Cout, 4, 4), generator=g) / (4 * Cin ** 0.5)
        ref = torch.nn.functional.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1)
        y, pre = ops.conv_transpose2d_fwd(x.cuda(), w.cuda(), b.cuda(), 1, want_preact=True)
        small, big = (lib.qarig_conv_transpose2d_workspace_bytes(Cin, Cout),
                      lib.qarig_conv_transpose2d_workspace_bytes_n(N, Cin, H, W, Cout))
    else:
        w = torch.randn((Cout, Cin, 3, 3), generator=g) / (3 * Cin ** 0.5)
        ref = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), padding=1)
        y, pre = ops.conv2d_fwd(x.cuda(), w.cuda(), b.cuda(), 1, 1, 1, want_preact=True)
        small, big = (lib.qarig_conv2d_fwd_workspace_bytes(Cin, Cout, 3),
                      lib.qarig_conv2d_fwd_workspace_bytes_n(N, Cin, H, W, Cout, 3, 1))
    assert rel_err(pre, ref) < 2e-6
    assert rel_err(y, torch.nn.functional.silu(ref)) < 4e-6
    if kind == "direct":
        assert big == small
        return
    assert big > small
    xc, wc, bc = x.cuda(), w.cuda(), b.cuda()
    y1 = torch.empty_like(y)
    ws = torch.empty(small, dtype=torch.uint8, device="cuda")
    if kind == "convt":
        rc = lib.qarig_conv_transpose2d_fwd(ptr(xc), N, Cin, H, W, ptr(wc), ptr(bc), Cout, 1, ptr(y1), None,
                                            ptr(ws), small, 0, _lib.stream())
    else:
        rc = lib.qarig_conv2d_fwd_ws(ptr(xc), N, Cin, H, W, ptr(wc), ptr(bc), Cout, 3, 1, 1, 1, ptr(y1), None,
                                     ptr(ws), small, 0, _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0 and rel_err(y1, y) < 5e-6 and not torch.equal(y1, y)


def test_decoder_four_images_readme_shape_vs_oracle_fp64():
    """The configuration tools/bench_generate.py times (4 latents of 32 x 32 x 4 -> 4 images): every layer of
    the README decoder takes a few-image launch form; pixels against the fp64 oracle at the 1e-5 target."""
    from models.FC_Decoder import FC_Decoder
    from oracle import ref_models as rm
    torch.manual_seed(5)
    dec = FC_Decoder(num_layers=2, image_channel=3, min_channel=256, max_channel=512, latent_channel=4)
    z = torch.tanh(torch.randn((4, 4, 32, 32), generator=torch.Generator().manual_seed(2)))
    sd64 = {k: v.double() for k, v in dec.state_dict().items()}
    ref = rm.fc_decoder(sd64, z.double())
    with torch.no_grad():
        y = dec.cuda()(z.cuda())
    assert y.shape == (4, 3, 128, 128) and rel_err(y, ref) < PIX_TOL


def test_inference_weight_copies_are_cached_and_follow_the_weights():
    """Under no_grad the tap-major weight copies are made once per weight and geometry
    (QARIG_CONV_PACKED_VALID on later calls); an in-place update of the weight (optimizer step,
    load_state_dict) must be seen by the next call."""
    from models.FC_Decoder import FC_Decoder
    from qarig import ops
    torch.manual_seed(7)
    dec = FC_Decoder(num_layers=1, image_channel=3, min_channel=128, max_channel=128, latent_channel=4).cuda().eval()
    z = torch.tanh(torch.randn(2, 4, 16, 16, device="cuda"))
    with torch.no_grad():
        y0 = dec(z)
        n_cached = len(ops._lp_cache)
        y1 = dec(z)                                  # second call: cached copies
        assert torch.equal(y0, y1) and len(ops._lp_cache) == n_cached and n_cached > 0
        assert dec(z[:1]).shape == (1, 3, 32, 32) and len(ops._lp_cache) > n_cached      # another geometry: its own copies
        for p in dec.parameters():
            p.mul_(1.5)                              # in place: version bump
        y2 = dec(z)
    fresh = FC_Decoder(num_layers=1, image_channel=3, min_channel=128, max_channel=128, latent_channel=4).cuda().eval()
    fresh.load_state_dict(dec.state_dict())
    with torch.no_grad():
        assert torch.equal(fresh(z), y2) and not torch.equal(y2, y0)
    # a kernel-family switch changes the copies' layout: entries made before it are not served after it
    from qarig import _lib
    with torch.no_grad():
        ya = dec(z)
        old = _lib.set_option("conv_ring", 0)
        try:
            yb = dec(z)                  # gather kernels, their own weight layout
        finally:
            _lib.set_option("conv_ring", old)
        assert rel_err(yb, ya) < 1e-5 and torch.equal(dec(z), ya)
    # training mode (grad enabled) never uses the cache: no new entries, and no launch is told that the packed
    # weights of an earlier call are still valid (flags = QARIG_CONV_PACKED_VALID) -- a write to the weights that
    # torch's version counter does not see (a broadcast into the flat buffer, a raw-pointer kernel) must not meet
    # stale copies in a training forward
    n = len(ops._lp_cache)
    seen = []
    real = ops._conv_workspace
    ops._conv_workspace = lambda *a, **k: (seen.append(real(*a, **k)) or seen[-1])
    try:
        dec(z).sum().backward()
    finally:
        ops._conv_workspace = real
    assert len(ops._lp_cache) == n and seen and all(flags == 0 for _, flags in seen)


@pytest.mark.parametrize("kind,N,Cin,H,W,Cout", [
    ("s1", 1, 128, 16, 16, 128),        # input gradient of a 3x3 / stride 1 layer: 2 tiles, split
    ("s1", 2, 512, 16, 16, 256),
    ("s2", 2, 128, 32, 32, 256),        # stride-2 forward: 4 tiles of 72 k-tiles
    ("s2", 1, 256, 32, 32, 128),
    ("convt", 2, 128, 16, 16, 128),     # ConvTranspose input gradient: 16-tap strided product over dT
    ("convt", 1, 256, 16, 16, 64)])
def test_few_image_backward_and_strided_launches_split_the_reduction(kind, N, Cin, H, W, Cout):
    """The input gradient of the 3x3 / stride 1 layers, the stride-2 forward and the ConvTranspose input gradient
    take the same k-tile windows on blockIdx.z as the stride-1 forward when their tiles alone leave CUs idle
    (config 1 trains at batch 4): forward and gradients against fp64 at the tolerances of the unsplit tests, and
    the scratch-size functions say that a split is planned."""
    from conftest import grad_err
    from qarig import functional as QF, _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(N * 5 + Cin + Cout)
    x = torch.randn((N, Cin, H, W), generator=g)
    if kind == "convt":
        w = torch.randn((Cin, Cout, 4, 4), generator=g) / (4 * Cin ** 0.5)
        f64 = lambda a, b, c: torch.nn.functional.conv_transpose2d(a, b, c, stride=2, padding=1)
        hip = lambda a, b, c: QF.conv_transpose2d_act(a, b, c, 0)
        assert lib.qarig_conv_transpose2d_bwd_data_workspace_bytes_n(N, Cin, H, W, Cout) > \
            lib.qarig_conv_transpose2d_workspace_bytes(Cin, Cout)
    else:
        st = 2 if kind == "s2" else 1
        w = torch.randn((Cout, Cin, 3, 3), generator=g) / (3 * Cin ** 0.5)
        f64 = lambda a, b, c: torch.nn.functional.conv2d(a, b, c, stride=st, padding=1)
        hip = lambda a, b, c: QF.conv2d_act(a, b, c, st, 1, 0)
        if kind == "s2":
            assert lib.qarig_conv2d_fwd_workspace_bytes_n(N, Cin, H, W, Cout, 3, 2) > \
                lib.qarig_conv2d_fwd_workspace_bytes(Cin, Cout, 3)
        else:
            assert lib.qarig_conv2d_bwd_data_workspace_bytes_n(N, Cin, H, W, Cout, 3, 1) > \
                lib.qarig_conv2d_bwd_data_workspace_bytes(Cin, Cout, 3)
    b = torch.randn(Cout, generator=g)
    a = [t.double().requires_grad_(True) for t in (x, w, b)]
    ya = f64(*a)
    dy = torch.randn(ya.shape, generator=g)
    (ya * dy.double()).sum().backward()
    c = [t.cuda().requires_grad_(True) for t in (x, w, b)]
    yc = hip(*c)
    assert rel_err(yc, ya) < 4e-6
    (yc * dy.cuda()).sum().backward()
    for p_, q_ in zip(c, a):
        assert grad_err(p_.grad, q_.grad) < 1e-5
