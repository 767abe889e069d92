"""The encoder's backward pass, Adam step, blend and export on the device (csrc/mjs_encoder_train.h,
mujoco_sim_amd.policies.DeviceEncoderOptimizer) against torch on the CPU. The bars and the mask route are _encoder_train_reference.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

import _critic_reference as cref
import _critic_train_reference as ctr
import _encoder_train_reference as R
from _visual_nets import cnn_forward, encoder_bar, make_cnn

gpu = pytest.mark.gpu
MODS = lambda cnn: (cnn.cnn[0], cnn.cnn[2], cnn.cnn[4], cnn.linear[0])  # noqa: E731


@pytest.fixture(scope="module")
def venv():
    """One seeded, reset Robot-Reach handle of 33 envs: the source of real frames, and the device the encoders live on."""
    import mujoco_sim_amd as m

    v = m.HipVectorEnv("robot_reach", 33, seed=11)
    v.reset()
    yield v
    v.close()


def case_images(venv, case):
    """Half real renders and half random bytes, uint8 [n, H, W, 3] on the device."""
    H, W, _, _ = case
    n = R.resolve_n(case)
    renders = venv.render(H, W)[: n - n // 2]
    assert renders.shape[0] == n - n // 2
    return torch.cat([renders, R.random_images(n // 2, H, W, R.case_seed(case) + 2).to(venv.device)]).contiguous()


def make(venv, case):
    from mujoco_sim_amd import DeviceEncoder, DeviceEncoderOptimizer

    cnn = R.case_cnn(case, device=venv.device)
    enc = DeviceEncoder.from_sb3(venv, cnn, case[0], case[1])
    return cnn, enc, DeviceEncoderOptimizer(enc)


def params_np(enc):
    """The packed copy as numpy arrays in torch layout (through export into fresh modules)."""
    cnn = make_cnn(enc.height, enc.width, enc.features_dim, seed=0, device=enc.device)
    enc.export(MODS(cnn))
    return [t.detach().cpu().numpy().copy() for m in MODS(cnn) for t in (m.weight, m.bias)]


# ---------------------------------------------------------------------------------------------- 1. gradients and masks
@gpu
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_gradients_and_masks(venv, case):
    H, W, F, _ = case
    n = R.resolve_n(case)
    ips, splits = R.split_rule(n, H, W, F)
    if case[3] == "multi":
        assert ips > 1 and splits > 1
    cnn, enc, opt = make(venv, case)
    images, dfeat = case_images(venv, case), R.make_dfeatures(case).to(venv.device)
    assert enc._lib.mjs_encoder_train_workspace_bytes(enc._e, n) == R.workspace_bytes(n, H, W, F)
    got = opt.gradients(images, dfeat)
    assert torch.equal(got["features"], enc.features(images))  # bit for bit
    # the masks and the stored activations against the plain float64 forward
    pre64, pre32 = R.plain_forward(cnn, images, torch.float64), R.plain_forward(cnn, images, torch.float32)
    masks = R.masks_of_activations(got["activations"], got["features"], H, W)
    R.check_masks(R.case_id(case), masks, pre64, pre32)
    (h1, w1), (h2, w2), (h3, w3) = R.geometry(H, W)
    stored = [got["activations"]["conv1"].cpu().reshape(n, h1, w1, 32).permute(0, 3, 1, 2), got["activations"]["conv2"].cpu().reshape(n, h2, w2, 64).permute(0, 3, 1, 2),
              got["activations"]["flat"].cpu().reshape(n, 64, h3, w3), got["features"].cpu()]
    for name, a, p64, p32 in zip(R.LAYERS, stored, pre64, pre32):
        e32, bar = encoder_bar(torch.relu(p64), torch.relu(p32))
        err = (a.double() - torch.relu(p64)).abs().max().item()
        print(f"{R.case_id(case)} {name} activations: kernel vs float64 {err:.3e}, torch float32 vs float64 {e32:.3e}, bar {bar:.3e}")
        assert err <= bar, (name, err, bar)
    # the gradients against both references under the kernel's own masks
    ref64, f64 = R.masked_backward(cnn, images, dfeat, masks, torch.float64)
    ref32, _ = R.masked_backward(cnn, images, dfeat, masks, torch.float32)
    R.check_grads(R.case_id(case), got["grads"], ref64, ref32)
    assert max(w.abs().max().item() for w, _ in ref64) > 1e-3  # the gradient is not all cut off by the ReLUs
    opt.close()
    enc.close()


# ---------------------------------------------------------------------------------------------- 2. the backward's index map
@gpu
def test_backward_index_map_known_answer(venv):
    from mujoco_sim_amd import DeviceEncoder, DeviceEncoderOptimizer

    H = W = 44
    n, F = 3, 4
    cnn = make_cnn(H, W, F, seed=1, device=venv.device)
    c1, c2, c3, fc = MODS(cnn)
    tap1, tap2, tap3 = (1, 2, 5), (1, 3), (2, 0)  # conv1 (c, ky, kx), conv2 (ky, kx), conv3 (ky, kx): test_index_map_known_answer's
    with torch.no_grad():
        for m in (c1, c2, c3, fc):
            m.weight.zero_()
            m.bias.zero_()
        c1.weight[0, tap1[0], tap1[1], tap1[2]] = 1.0
        c2.weight[0, 0, tap2[0], tap2[1]] = 1.0
        c3.weight[0, 0, tap3[0], tap3[1]] = 1.0
        for f in range(F):
            fc.weight[f, f] = 1.0
    enc = DeviceEncoder.from_sb3(venv, cnn, H, W)
    opt = DeviceEncoderOptimizer(enc)
    images = R.random_images(n, H, W, seed=4400).to(venv.device)  # random bytes: neighbouring pixels differ
    x = images.cpu().numpy().astype(np.float32) / np.float32(255.0)  # [n, y, x, c]
    img, (y3, x3) = 1, (1, 0)
    dfeat = torch.zeros(n, F, device=venv.device)
    dfeat[img, y3 * 2 + x3] = 1.0  # feature f = channel 0 of the CHW flatten at conv3's output position (y3, x3)
    y2, x2 = y3 + tap3[0], x3 + tap3[1]          # the one conv2 output position the gradient reaches
    y1, x1 = 2 * y2 + tap2[0], 2 * x2 + tap2[1]  # the one conv1 output position
    assert x[img, 4 * y1 + tap1[1], 4 * x1 + tap1[2], tap1[0]] > 0  # the chain's unit is on
    got = opt.gradients(images, dfeat)["grads"]
    (dw1, db1), (dw2, db2), (dw3, db3), (dwf, dbf) = [(w.cpu().numpy(), b.cpu().numpy()) for w, b in got]
    # dW_conv1[0, c, ky, kx] is the pixel (4 y1 + ky, 4 x1 + kx, c) of image `img`; every other output channel gets nothing
    want1 = np.zeros((32, 3, 8, 8), np.float32)
    want1[0] = x[img, 4 * y1: 4 * y1 + 8, 4 * x1: 4 * x1 + 8, :].transpose(2, 0, 1)
    assert np.array_equal(dw1, want1) and len(np.unique(want1)) > 100
    assert np.array_equal(db1, np.eye(32, dtype=np.float32)[0])
    # dW_conv2[0, 0, ky, kx] is conv1's channel 0 at (2 y2 + ky, 2 x2 + kx): the pixel under conv1's tap there
    want2 = np.zeros((64, 32, 4, 4), np.float32)
    for ky in range(4):
        for kx in range(4):
            want2[0, 0, ky, kx] = x[img, 4 * (2 * y2 + ky) + tap1[1], 4 * (2 * x2 + kx) + tap1[2], tap1[0]]
    assert np.array_equal(dw2, want2) and np.array_equal(db2, np.eye(64, dtype=np.float32)[0])
    # dW_conv3[0, 0, ky, kx] is conv2's channel 0 at (y3 + ky, x3 + kx)
    want3 = np.zeros((64, 64, 3, 3), np.float32)
    for ky in range(3):
        for kx in range(3):
            yy, xx = 2 * (y3 + ky) + tap2[0], 2 * (x3 + kx) + tap2[1]
            want3[0, 0, ky, kx] = x[img, 4 * yy + tap1[1], 4 * xx + tap1[2], tap1[0]]
    assert np.array_equal(dw3, want3) and np.array_equal(db3, np.eye(64, dtype=np.float32)[0])
    # dW_fc[f] is image `img`'s flat row
    flat = enc.features(images).cpu().numpy()  # features f = flat[f] here (identity rows), f < 4 = channel 0's four positions
    wantf = np.zeros((F, 256), np.float32)
    wantf[y3 * 2 + x3, :4] = flat[img]
    assert np.array_equal(dwf, wantf) and np.array_equal(dbf, np.eye(F, dtype=np.float32)[y3 * 2 + x3])
    opt.close()
    enc.close()


# ---------------------------------------------------------------------------------------------- 3. reproducibility
@gpu
def test_gradients_and_steps_are_reproducible(venv):
    case = (44, 44, 33, "multi")
    images, dfeat = case_images(venv, case), R.make_dfeatures(case).to(venv.device)
    runs = []
    for _ in range(2):
        cnn, enc, opt = make(venv, case)
        g1 = [t.clone() for pair in opt.gradients(images, dfeat)["grads"] for t in pair]
        g2 = [t.clone() for pair in opt.gradients(images, dfeat)["grads"] for t in pair]
        assert all(torch.equal(a, b) for a, b in zip(g1, g2))  # two calls
        for _ in range(2):
            opt.step(images, dfeat)
        runs.append((g1, params_np(enc)))
        opt.close()
        enc.close()
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))  # two optimisers on copies
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


# ---------------------------------------------------------------------------------------------- 4. Adam
@gpu
@pytest.mark.parametrize("case", [(36, 52, 40, 17), (44, 44, 33, "multi")], ids=R.case_id)
def test_adam_is_its_float32_restatement_on_the_kernel_s_gradients(venv, case):
    cnn, enc, opt = make(venv, case)
    images = case_images(venv, case)
    p = params_np(enc)
    m, v = [np.zeros_like(a) for a in p], [np.zeros_like(a) for a in p]
    g = torch.Generator().manual_seed(5)
    for t in range(1, 4):
        dfeat = torch.randn(images.shape[0], case[2], generator=g).to(venv.device)
        grads = [a.cpu().numpy() for pair in opt.gradients(images, dfeat)["grads"] for a in pair]
        opt.step(images, dfeat)
        assert opt.step_count == t
        for k in range(8):
            p[k], m[k], v[k] = ctr.adam_step32(p[k], grads[k], m[k], v[k], t)
        now = params_np(enc)
        for k in range(8):
            assert np.array_equal(now[k], p[k]), (t, k, np.abs(now[k] - p[k]).max())
    opt.close()
    enc.close()


# ---------------------------------------------------------------------------------------------- 5. a zero gradient moves nothing
@gpu
def test_zero_dfeatures_moves_nothing(venv):
    case = (36, 52, 40, 17)
    cnn, enc, opt = make(venv, case)
    images = case_images(venv, case)
    before = params_np(enc)
    opt.step(images, torch.zeros(17, 40, device=venv.device))
    assert opt.step_count == 1
    for a, b in zip(before, params_np(enc)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    opt.close()
    enc.close()


# ---------------------------------------------------------------------------------------------- 6. export round trip, padding
@gpu
def test_export_round_trip_and_padding(venv):
    from mujoco_sim_amd import DeviceEncoder

    case = (44, 44, 33, 17)
    cnn, enc, opt = make(venv, case)
    images, dfeat = case_images(venv, case), R.make_dfeatures(case).to(venv.device)
    for _ in range(3):
        opt.step(images, dfeat)
    trained = enc.features(images).clone()
    stale = cnn_forward(cnn, images, torch.float32)
    assert (trained.cpu() - stale).abs().max().item() > 1e-4  # the steps moved the parameters; the modules are stale
    enc.export()
    again = DeviceEncoder.from_sb3(venv, cnn, 44, 44)
    assert torch.equal(again.features(images), trained)  # bit for bit
    # the trained copy and the copy packed from the exported modules hold the same real entries: (1 - tau) * p + tau * p == p exactly.
    # (The padding - fc's outputs 33..63 - has Gf = 0, hence g = m = v = 0 and p = 0 - 0 / eps; no entry point reads it back.)
    enc.blend_from(again, 0.5)
    assert torch.equal(enc.features(images), trained)
    fresh = make_cnn(44, 44, 33, seed=77, device=venv.device)
    other = DeviceEncoder.from_sb3(venv, fresh, 44, 44)
    other.blend_from(enc, 1.0)  # the whole packed copy, padding included, into another encoder ...
    out = make_cnn(44, 44, 33, seed=78, device=venv.device)
    other.export(MODS(out))     # ... whose export matches
    for a, b in zip(MODS(out), MODS(cnn)):
        assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)
    for e in (opt, enc, again, other):
        e.close()


# ---------------------------------------------------------------------------------------------- 7. blend
@gpu
def test_blend_from_matches_the_restatement(venv):
    from mujoco_sim_amd import DeviceEncoder

    H, W, F = 36, 52, 40
    a, b = make_cnn(H, W, F, seed=21, device=venv.device), make_cnn(H, W, F, seed=22, device=venv.device)
    dst, src = DeviceEncoder.from_sb3(venv, a, H, W), DeviceEncoder.from_sb3(venv, b, H, W)
    tau = 0.005
    dst.blend_from(src, tau)
    got = params_np(dst)
    t, omt = np.float32(tau), np.float32(1.0 - tau)
    for k, (ma, mb) in enumerate(zip(MODS(a), MODS(b))):
        for j, name in enumerate(("weight", "bias")):
            d, s = getattr(ma, name).detach().cpu().numpy(), getattr(mb, name).detach().cpu().numpy()
            want = (np.float64(t) * s.astype(np.float64) + (omt * d).astype(np.float64)).astype(np.float32)  # pack_lerp_np's blend
            assert np.array_equal(got[2 * k + j], want), (k, name)
    # the linear layer through pack_lerp_np itself
    K, O = 64 * 3, cref.round_up(F, 32)
    w0, b0 = cref.pack_lerp_np(None, None, MODS(a)[3].weight.detach().cpu().numpy(), MODS(a)[3].bias.detach().cpu().numpy(), K, O, 1.0)
    w1, b1 = cref.pack_lerp_np(w0, b0, MODS(b)[3].weight.detach().cpu().numpy(), MODS(b)[3].bias.detach().cpu().numpy(), K, O, tau)
    assert np.array_equal(w1[:, :F].T, got[6]) and np.array_equal(b1[:F], got[7])
    dst.blend_from(src, 1.0)  # tau = 1 copies
    for x, y in zip(params_np(dst), params_np(src)):
        assert np.array_equal(x, y)
    with pytest.raises(ValueError, match="shape"):
        dst.blend_from(DeviceEncoder.from_sb3(venv, make_cnn(36, 36, F, seed=1, device=venv.device), 36, 36), 0.5)
    with pytest.raises(ValueError, match="tau"):
        dst.blend_from(src, 0.0)
    dst.close()
    src.close()


# ---------------------------------------------------------------------------------------------- 8. a small regression
@gpu
def test_small_regression_follows_torch(venv):
    from mujoco_sim_amd import DeviceEncoder, DeviceEncoderOptimizer

    cfg = R.REG
    cnn, head, images, targets = R.regression_setup()
    l64, d32 = R.regression_references()
    dev = venv.device
    cnn, head, images, targets = cnn.to(dev), head.to(dev), images.to(dev), targets.to(dev)
    enc = DeviceEncoder.from_sb3(venv, cnn, cfg["H"], cfg["W"])
    opt = DeviceEncoderOptimizer(enc, lr=cfg["lr"])
    head_opt = torch.optim.Adam(head.parameters(), lr=cfg["lr"])
    losses = []
    for _ in range(cfg["steps"]):
        f = enc.features(images).requires_grad_(True)
        loss = torch.nn.functional.mse_loss(head(f), targets)
        head_opt.zero_grad()
        loss.backward()
        head_opt.step()
        opt.step(images, f.grad.contiguous())
        losses.append(loss.item())
    losses = np.array(losses)
    d = float(np.max(np.abs(losses - l64) / np.abs(l64)))
    print(f"regression: device vs float64 {d:.3e}, torch float32 vs float64 {d32:.3e}, ratio {d / d32:.2f}; loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses[-1] < 0.5 * losses[0]
    assert d <= 4 * d32, (d, d32)
    opt.close()
    enc.close()


# ---------------------------------------------------------------------------------------------- 9. native refusals
@gpu
def test_native_refusals(venv):
    from mujoco_sim_amd import DeviceEncoder, DeviceEncoderOptimizer
    from mujoco_sim_amd import _native as nat

    L = nat.lib()
    INVALID = -1
    dev, s = venv.device, venv._stream()
    err = lambda: L.mjs_last_error(None)  # noqa: E731
    cnn = make_cnn(36, 36, 8, seed=2, device=dev)
    enc, enc2 = DeviceEncoder.from_sb3(venv, cnn, 36, 36), DeviceEncoder.from_sb3(venv, cnn, 36, 36)
    opt = DeviceEncoderOptimizer(enc)
    n = 5
    images = torch.zeros(n, 36, 36, 3, dtype=torch.uint8, device=dev)
    dfeat = torch.ones(n, 8, device=dev)
    ws = torch.full((L.mjs_encoder_train_workspace_bytes(enc._e, n) // 4,), 7.0, device=dev)
    feat = torch.full((n, 8), 7.0, device=dev)
    grads = enc._empty_like_parameters()
    for t in grads:
        t.fill_(7.0)
    before = params_np(enc)

    def args(**kw):
        base = dict(n=n, rgb_dev=images.data_ptr(), dfeatures_dev=dfeat.data_ptr(), workspace_dev=ws.data_ptr(), features_out_dev=feat.data_ptr())
        base.update(kw)
        return nat.MjsEncoderGradArgs(**base)

    def untouched():
        torch.cuda.synchronize()
        assert bool((ws == 7.0).all()) and bool((feat == 7.0).all()) and all(bool((t == 7.0).all()) for t in grads)
        assert opt.step_count == 0
        for a, b in zip(before, params_np(enc)):
            assert np.array_equal(a, b)

    grad = lambda a, e=enc._e, o=opt._o: L.mjs_encoder_grad(e, o, C.byref(a) if a is not None else None, s)  # noqa: E731
    update = lambda a, lr=1e-3, o=opt._o: L.mjs_encoder_update(o, C.byref(a) if a is not None else None, lr, s)  # noqa: E731
    # null pointers
    assert grad(args(), e=None) == INVALID and b"null" in err()
    assert grad(args(), o=None) == INVALID and grad(None) == INVALID and update(args(), o=None) == INVALID and update(None) == INVALID
    for field in ("rgb_dev", "dfeatures_dev", "workspace_dev"):
        assert grad(args(**{field: None})) == INVALID and b"null" in err(), field
        assert update(args(**{field: None})) == INVALID, field
    # a wrong struct_size, n < 0
    assert grad(args(struct_size=8)) == INVALID and b"struct_size" in err() and update(args(struct_size=8)) == INVALID
    assert grad(args(n=-1)) == INVALID and b"negative" in err() and update(args(n=-1)) == INVALID
    # an optimiser of another encoder
    assert grad(args(), e=enc2._e) == INVALID and b"another encoder" in err()
    # lr < 0, grads_out in an update, an incomplete grads_out
    assert update(args(), lr=-1.0) == INVALID and b"lr" in err()
    w = enc._weights_struct(grads)
    assert update(args(grads_out=C.pointer(w))) == INVALID and b"grads_out" in err()
    assert grad(args(grads_out=C.pointer(nat.MjsEncoderWeights()))) == INVALID and b"null" in err()
    assert grad(args(grads_out=C.pointer(nat.MjsEncoderWeights(struct_size=8)))) == INVALID
    # an encoder that was never loaded: no optimiser, no export, no blend source
    raw = C.c_void_p()
    assert L.mjs_encoder_create(C.byref(nat.MjsEncoderDesc(device=venv._dev_index, height=36, width=36, channels=3, features_dim=8)), C.byref(raw)) == 0
    o2 = C.c_void_p()
    desc = lambda **kw: C.byref(nat.MjsEncoderOptDesc(**{**dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8), **kw}))  # noqa: E731
    assert L.mjs_encoder_opt_create(raw, desc(), C.byref(o2)) == INVALID and b"mjs_encoder_load" in err() and not o2.value
    assert L.mjs_encoder_export(raw, C.byref(w), s) == INVALID and b"mjs_encoder_load" in err()
    assert L.mjs_encoder_blend(enc._e, raw, 0.5, s) == INVALID and b"mjs_encoder_load" in err()
    # the optimiser's descriptor
    for kw in (dict(struct_size=8), dict(lr=-1.0), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(eps=0.0)):
        assert L.mjs_encoder_opt_create(enc._e, desc(**kw), C.byref(o2)) == INVALID and len(err()) > 0 and not o2.value, kw
    assert L.mjs_encoder_opt_create(None, desc(), C.byref(o2)) == INVALID and L.mjs_encoder_opt_create(enc._e, None, C.byref(o2)) == INVALID
    assert L.mjs_encoder_opt_create(enc._e, desc(), None) == INVALID
    # the blend: shapes, tau, tau != 1 into an encoder never loaded
    big = DeviceEncoder.from_sb3(venv, make_cnn(44, 44, 8, seed=3, device=dev), 44, 44)
    assert L.mjs_encoder_blend(enc._e, big._e, 0.5, s) == INVALID and b"shape" in err()
    for tau in (0.0, -0.5, 1.5, float("nan")):
        assert L.mjs_encoder_blend(enc._e, enc2._e, tau, s) == INVALID and b"tau" in err(), tau
    assert L.mjs_encoder_blend(raw, enc._e, 0.5, s) == INVALID and b"tau" in err()
    assert L.mjs_encoder_blend(None, enc._e, 0.5, s) == INVALID and L.mjs_encoder_blend(enc._e, None, 0.5, s) == INVALID
    # the export
    assert L.mjs_encoder_export(None, C.byref(w), s) == INVALID and L.mjs_encoder_export(enc._e, None, s) == INVALID
    assert L.mjs_encoder_export(enc._e, C.byref(nat.MjsEncoderWeights(struct_size=8)), s) == INVALID and b"struct_size" in err()
    assert L.mjs_encoder_export(enc._e, C.byref(nat.MjsEncoderWeights()), s) == INVALID and b"null" in err()
    assert L.mjs_encoder_train_workspace_bytes(None, 5) == 0 and L.mjs_encoder_train_workspace_bytes(enc._e, 0) == 0 and L.mjs_encoder_train_workspace_bytes(enc._e, -1) == 0
    # n == 0 does nothing
    assert grad(args(n=0)) == 0 and update(args(n=0)) == 0
    untouched()
    # ... and the accepted calls do launch
    assert L.mjs_encoder_blend(raw, enc._e, 1.0, s) == 0  # tau == 1 into an encoder never loaded: a copy
    assert grad(args(grads_out=C.pointer(w))) == 0
    torch.cuda.synchronize()
    assert bool((feat != 7.0).any()) and all(bool((t != 7.0).any()) for t in grads)
    L.mjs_encoder_destroy(raw)
    L.mjs_encoder_opt_destroy(None)
    for e in (opt, enc, enc2, big):
        e.close()
