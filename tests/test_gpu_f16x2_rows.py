"""The matrix kernels on the two-term f16 split (csrc/f16split.h) held to a bar PER ROW, against float64 (tests/row_bars.py): kernels Z, G,
R, RB, RS, RV on the forwards and data gradients of Linear(3136, 512) and of conv layers 2 / 3 (row = sample / image), kernels V, U, W, Y, H
and the layer-1 kernel on the weight gradients (row = output channel of dW), each on its own route.

tests/test_gpu_f16x2.py holds the same kernels to 2e-5 of the TENSOR's largest value: with rows over 2^-12 .. 2^-16, as PPO's per-sample
gradients are, that accepts relative errors above 1e-3 on most rows -- a kernel that lost its lo terms altogether passes it everywhere below
6 % of the tensor's maximum.  Here every row answers for itself: ``err_r <= (c rho32 + 2^-22) scale_r``, rho32 = torch f32's own row-relative
error against float64 on the CPU over a batch of at least 64 rows / 8 images of the recipe (the kernel gets the first rows of that batch), c
per kernel family in tests/row_bars.py.  tests/test_row_bars_model.py shows on the CPU what this bar accepts and rejects.

Every case prints its worst ratio (err_r / scale_r) / rho32 (DESIGN.md keeps the table) and checks run-to-run bit equality once."""
import pytest
import torch

import row_bars as rb

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from cleanrl_amd import cnn

DEV = torch.device("cuda:0")
SWITCHES = ("MI355PPO_CONV_R", "MI355PPO_CONV_RB", "MI355PPO_CONV_RS", "MI355PPO_CONV_RV", "MI355PPO_CONV_U", "MI355PPO_FC_G", "MI355PPO_FC_H")


def _env(monkeypatch, **env):
    for key in SWITCHES:
        monkeypatch.delenv(key, raising=False)
    for key, val in env.items():
        monkeypatch.setenv("MI355PPO_" + key, val)


def _rec_of(x):
    r = cnn.new_amax(1, x.device)[0]
    cnn.absmax(x.contiguous(), r)
    return r


def _padded(t, pitch):
    """(rows, cols) CPU tensor -> a device view with row pitch ``pitch``."""
    out = torch.zeros((t.shape[0], pitch), device=DEV)[:, :t.shape[1]]
    out.copy_(t)
    return out


def _report(what, ratio, c):
    print(f"row-bar ratio | {what} | {ratio:.2f} | c = {c:g}")


# ------------------------------------------------------------------------------------------------------------ FC forward and data gradient
@pytest.mark.parametrize("route", ["wrapper", "Z", "G"])
@pytest.mark.parametrize("M", [1, 5, 77, 300])
def test_fc_forward_and_data_gradient_rows(monkeypatch, M, route):
    """Linear(3136, 512) forward (bias + ReLU) and data gradient (a padded dz pitch of 516, conv3's ReLU mask as bits): through the wrapper
    (below 8,192 rows the forward splits K over the grid and folds the partials), through the C ABI without a workspace (kernel Z over the
    whole K) and on kernel G (MI355PPO_FC_G=min:1)."""
    case = rb.fc_case(M)
    lib = cnn._lib.load()
    _env(monkeypatch, **({"FC_G": "min:1"} if route == "G" else {"FC_G": "0"} if route == "Z" else {}))
    if route != "wrapper":
        assert chr(lib.mi355ppo_fc_packed_kernel_f16x2(M, 512, 3136, 0)) == route and chr(lib.mi355ppo_fc_packed_kernel_f16x2(M, 3136, 512, 1)) == route
    a, W, b = case.a[:M].to(DEV), case.W.to(DEV), case.b.to(DEV)
    pack, ra = cnn.fc_pack_f16x2(W), _rec_of(a)

    def forward():
        if route == "wrapper":
            assert lib.mi355ppo_fc_fwd_workspace_bytes(M, 512, 3136) > 0             # (the K-split route)
            return cnn.fc_fwd_relu_packed(a, pack, b, 512, out=torch.full((M, 512), float("nan"), device=DEV), amax=(ra, cnn.new_amax(1, DEV)[0]))
        h, rh = torch.full((M, 512), float("nan"), device=DEV), cnn.new_amax(1, DEV)[0]
        st = lib.mi355ppo_fc_fwd_relu_packed_f16x2_f32(cnn._ptr(a), 3136, cnn._ptr(pack), cnn._ptr(b), cnn._ptr(h), M, 512, 3136, None, 0, cnn._ptr(ra),
                                                       cnn._ptr(rh), None)
        assert st == 0, lib.mi355ppo_last_error()
        torch.cuda.synchronize()                             # (rh stays alive until the kernel has written it)
        return h

    h = forward()
    c_fwd = rb.C_FC_FORWARD_SPLIT_K if route == "wrapper" else rb.C_FC_FORWARD
    _report(f"fc forward, route {route}, M = {M}", rb.row_bar(f"fc forward, route {route}, M={M}", h, case.h64[:M], case.h32, case.h64, c=c_fwd), c_fwd)
    assert torch.equal(h.view(torch.int32), forward().view(torch.int32))
    dz = _padded(case.dz[:M], 516)
    packt = cnn.fc_pack_f16x2(_padded(case.W.t(), 516))
    bits, rz = rb.packed_bits(case.mask[:M].to(DEV)), _rec_of(dz)

    def dgrad():
        return cnn.fc_dgrad_mask_packed(dz, packt, a, out=torch.full((M, 3136), float("nan"), device=DEV), bits=bits, amax=(rz, cnn.new_amax(1, DEV)[0]))

    da = dgrad()
    _report(f"fc data gradient, route {route}, M = {M}", rb.row_bar(f"fc data gradient, route {route}, M={M}", da, case.da64[:M], case.da32, case.da64, c=rb.C_DGRAD),
            rb.C_DGRAD)
    assert torch.equal(da.view(torch.int32), dgrad().view(torch.int32))


# --------------------------------------------------------------------------------------------- conv layers 2 / 3, forward and data gradient
FWD_ROUTES = {"Z": {"CONV_R": "0"}, "R": {"CONV_R": "min:1", "CONV_RS": "0"}, "RS": {"CONV_R": "min:1", "CONV_RS": "min:1"}}
DGRAD_ROUTES = {"Z": {"CONV_R": "0"}, "R": {"CONV_R": "min:1", "CONV_RB": "0", "CONV_RV": "0"}, "RB": {"CONV_R": "min:1", "CONV_RB": "min:1"},
                "RV": {"CONV_R": "min:1", "CONV_RV": "min:1"}}
CONV_CASES = ([(layer, "Z", n) for layer in (2, 3) for n in (1, 3, 37, 773)]             # (773: the first partial 64-row tile past 768 images)
              + [(layer, "R", n) for layer in (2, 3) for n in (1, 3, 37)])


@pytest.mark.parametrize("layer,route,images", CONV_CASES + [(2, "RS", n) for n in (1, 3, 37)])
def test_conv_forward_rows(monkeypatch, layer, route, images):
    """Kernel Z (32-row tiles below 768 images without the mask bits, 64-row tiles with them and above), kernel R, and kernel RS on layer 2
    (MI355PPO_CONV_RS=min:1): per image, with and without the mask-bit epilogue."""
    case = rb.conv_case(layer, images)
    lib = cnn._lib.load()
    _env(monkeypatch, **FWD_ROUTES[route])
    assert chr(lib.mi355ppo_cnn_conv_packed_kernel_f16x2(images, layer, 0)) == ("Z" if route == "Z" else "R")
    x, b = case.x[:images].to(DEV), case.b.to(DEV)
    pack, rx = cnn.conv_zpack_f16x2(case.W.to(DEV), layer, cnn.MODE_FWD), _rec_of(x)
    y = cnn.conv_fwd_packed(x, pack, b, layer, amax=(rx, cnn.new_amax(1, DEV)[0]))
    bits = torch.empty(cnn.mask_words(y.numel()), dtype=torch.int32, device=DEV)
    yb = cnn.conv_fwd_packed(x, pack, b, layer, bits=bits, amax=(rx, cnn.new_amax(1, DEV)[0]))
    for got, what in ((y, "no bits"), (yb, "mask bits")):
        name = f"conv{layer} forward, route {route}, {images} images, {what}"
        _report(name, rb.row_bar(name, got, case.y64[:images], case.y32, case.y64, c=rb.C_CONV_FORWARD), rb.C_CONV_FORWARD)
    assert torch.equal(cnn.unpack_mask_bits(bits, yb.shape), yb > 0)
    assert torch.equal(y.view(torch.int32), cnn.conv_fwd_packed(x, pack, b, layer, amax=(rx, cnn.new_amax(1, DEV)[0])).view(torch.int32))


@pytest.mark.parametrize("layer,route,images", CONV_CASES + [(2, "RB", n) for n in (1, 3, 37)] + [(3, "RV", n) for n in (1, 3, 37)])
def test_conv_data_gradient_rows(monkeypatch, layer, route, images):
    """Kernel Z (the mask as ``act`` and as bits), kernel R, kernel RB on layer 2 (MI355PPO_CONV_RB=min:1) and kernel RV on layer 3
    (MI355PPO_CONV_RV=min:1; the resident kernels take the mask as bits only): per image."""
    case = rb.conv_case(layer, images)
    lib = cnn._lib.load()
    _env(monkeypatch, **DGRAD_ROUTES[route])
    assert chr(lib.mi355ppo_cnn_conv_packed_kernel_f16x2(images, layer, 1)) == {"Z": "Z", "R": "R", "RB": "B", "RV": "R"}[route]
    dz, act = case.dz[:images].to(DEV), case.act[:images].to(DEV)
    pack = cnn.conv_zpack_f16x2(case.W.to(DEV), layer, cnn.MODE_DGRAD_S2 if layer == 2 else cnn.MODE_DGRAD_S1)
    bits, rz = rb.packed_bits(act > 0), _rec_of(dz)
    got = cnn.conv_dgrad_packed(dz, pack, None, layer, bits=bits, amax=(rz, cnn.new_amax(1, DEV)[0]))
    name = f"conv{layer} data gradient, route {route}, {images} images, mask bits"
    _report(name, rb.row_bar(name, got, case.dx64[:images], case.dx32, case.dx64, c=rb.C_DGRAD), rb.C_DGRAD)
    assert torch.equal(got.view(torch.int32), cnn.conv_dgrad_packed(dz, pack, None, layer, bits=bits, amax=(rz, cnn.new_amax(1, DEV)[0])).view(torch.int32))
    if route == "Z":
        got = cnn.conv_dgrad_packed(dz, pack, act, layer, amax=(rz, cnn.new_amax(1, DEV)[0]))
        name = f"conv{layer} data gradient, route {route}, {images} images, mask from act"
        _report(name, rb.row_bar(name, got, case.dx64[:images], case.dx32, case.dx64, c=rb.C_DGRAD), rb.C_DGRAD)


# ----------------------------------------------------------------------------------------------------------------------- weight gradients
@pytest.mark.parametrize("layer,images,kernel", [(2, 16, "U"), (2, 208, "U"), (2, 256, "U"), (2, 208, "V"), (2, 256, "V"),
                                                 (3, 1, "U"), (3, 5, "U"), (3, 304, "U"), (3, 304, "V")])
def test_conv_weight_gradient_rows(monkeypatch, layer, images, kernel):
    """Kernel U (the default) and kernel V (MI355PPO_CONV_U=0; multiples of 16 images with work for every slab: from 208 / 304 images on) on
    layers 2 / 3: per output channel of dW against
    torch f32's conv2d_weight on the CPU; the bias gradient through the same bar."""
    case = rb.conv_wgrad_case(layer, images)
    lib = cnn._lib.load()
    _env(monkeypatch, **({"CONV_U": "0"} if kernel == "V" else {}))
    assert chr(lib.mi355ppo_cnn_conv_wgrad_kernel_f16x2(images, layer)) == kernel
    src, dz = case.src[:images].to(DEV), case.dz[:images].to(DEV)
    rs, rz = _rec_of(src), _rec_of(dz)
    dW, db = cnn.conv_wgrad(src, dz, layer, amax=(rs, rz))
    name = f"conv{layer} weight gradient, kernel {kernel}, {images} images"
    _report(name, rb.row_bar(name, dW, case.dW64, case.dW32_yard, case.dW64_yard, c=rb.C_WGRAD), rb.C_WGRAD)
    _report(name + ", bias", rb.row_bar(name + ", bias", db, case.db64, case.db32_yard, case.db64_yard, c=rb.C_BIAS_GRAD), rb.C_BIAS_GRAD)
    dW2, db2 = cnn.conv_wgrad(src, dz, layer, amax=(rs, rz))
    assert torch.equal(dW.view(torch.int32), dW2.view(torch.int32)) and torch.equal(db.view(torch.int32), db2.view(torch.int32))


@pytest.mark.parametrize("images", [8, 300])
def test_conv1_weight_gradient_rows(monkeypatch, images):
    """The layer-1 weight gradient of the f16 split through a row gather of uint8 frames: per output channel."""
    case = rb.conv1_wgrad_case(images)
    lib = cnn._lib.load()
    _env(monkeypatch)
    assert chr(lib.mi355ppo_cnn_conv_wgrad_kernel_f16x2(images, 1)) == "U"
    obs, inds, dz = case.src.to(DEV), case.inds[:images].to(DEV), case.dz[:images].to(DEV)
    rz = _rec_of(dz)
    dW, db = cnn.conv_wgrad(obs, dz, 1, inds, amax=(None, rz))
    name = f"conv1 weight gradient, kernel U, {images} images"
    _report(name, rb.row_bar(name, dW, case.dW64, case.dW32_yard, case.dW64_yard, c=rb.C_WGRAD), rb.C_WGRAD)
    _report(name + ", bias", rb.row_bar(name + ", bias", db, case.db64, case.db32_yard, case.db64_yard, c=rb.C_BIAS_GRAD), rb.C_BIAS_GRAD)
    dW2, db2 = cnn.conv_wgrad(obs, dz, 1, inds, amax=(None, rz))
    assert torch.equal(dW.view(torch.int32), dW2.view(torch.int32)) and torch.equal(db.view(torch.int32), db2.view(torch.int32))


@pytest.mark.parametrize("M,kernel", [(1000, "Y"), (1024, "W"), (1000, "H")])
def test_fc_weight_gradient_rows(monkeypatch, M, kernel):
    """Linear(3136, 512)'s weight gradient ``dz.T @ a`` (a padded dz pitch): kernel Y at 1,000 rows, kernel W at 1,024, kernel H forced
    (MI355PPO_FC_H=min:1) at 1,000 -- per output unit against torch f32's matmul on the CPU."""
    case = rb.fc_wgrad_case(M)
    lib = cnn._lib.load()
    _env(monkeypatch, **({"FC_H": "min:1"} if kernel == "H" else {"FC_H": "0"}))
    assert chr(lib.mi355ppo_fc_wgrad_kernel_f16x2(M, 512, 3136)) == kernel
    a, dz = case.a[:M].to(DEV), _padded(case.dz[:M], 516)
    rz, ra = _rec_of(dz), _rec_of(a)
    got = cnn.fc_wgrad(dz, a, amax=(rz, ra), out=torch.full((512, 3136), float("nan"), device=DEV))
    name = f"fc weight gradient, kernel {kernel}, M = {M}"
    _report(name, rb.row_bar(name, got, case.dW64, case.dW32_yard, case.dW64_yard, c=rb.C_WGRAD), rb.C_WGRAD)
    assert torch.equal(got.view(torch.int32), cnn.fc_wgrad(dz, a, amax=(rz, ra)).view(torch.int32))
