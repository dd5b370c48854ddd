"""Shared checks of the forward-only mode (GSR_FORWARD_ONLY, include/gsr.h) for the emulator tests (test_forward_only.py) and the
GPU tests (test_gpu_forward_only.py): the same scene through gsr_forward with and without the bit, through the Python boundary
(rasterize_points.RasterizeGaussiansCUDA) on either library."""
import numpy as np
import torch

from photo_slam_amd import capi
from photo_slam_amd import rasterize_points as rp

FORWARD_ONLY = capi.FORWARD_ONLY


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class RecordingWorkspace(rp.RasterWorkspace):
    """rasterize_points.RasterWorkspace that remembers the sizes gsr_forward asked for (geometry, binning, image)"""

    def __init__(self):
        super().__init__()
        self.requested = [None, None, None]

    def taker(self, i, dev):
        inner = super().taker(i, dev)

        def fn(ctx, nbytes):
            self.requested[i] = int(nbytes)
            return inner(ctx, nbytes)
        cb = capi.ALLOC_FN(fn)
        cb._inner = inner   # (keeps the wrapped callback alive)
        return cb


def inputs(cl, cam, bg, dev, use_colors_precomp=False, use_cov3D_precomp=False, sh=None):
    """keyword arguments of RasterizeGaussiansCUDA for the cloud and camera (activated parameters, as the parity tests)"""
    empty = torch.empty(0, device=dev)
    P = cl.xyz.shape[0]
    rng = np.random.default_rng(P)
    colors = rng.random((P, 3)).astype(np.float32)
    if use_cov3D_precomp:
        s = cl.get_scaling().astype(np.float64)
        q = cl.get_rotation().astype(np.float64)
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                      2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                      2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
        M = R * s[:, None, :]
        S = M @ M.transpose(0, 2, 1)
        cov = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)
    return dict(background=_t(bg, dev), means3D=_t(cl.xyz, dev),
                colors=_t(colors, dev) if use_colors_precomp else empty, opacity=_t(cl.get_opacity(), dev),
                scales=empty if use_cov3D_precomp else _t(cl.get_scaling(), dev),
                rotations=empty if use_cov3D_precomp else _t(cl.get_rotation(), dev), scale_modifier=1.0,
                cov3D_precomp=_t(cov, dev) if use_cov3D_precomp else empty, viewmatrix=_t(cam.viewmatrix, dev),
                projmatrix=_t(cam.projmatrix, dev), tan_fovx=cam.tanfovx, tan_fovy=cam.tanfovy, image_height=cam.H,
                image_width=cam.W, sh=empty if use_colors_precomp else (sh if sh is not None else _t(cl.get_features(), dev)),
                degree=3, campos=_t(cam.campos, dev), prefiltered=False)


def render(lib_path, a, flags, sh_adam=None):
    """(R, image, radii, workspace with the requested sizes, forward_only flag of the call) of one gsr_forward"""
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        ws = RecordingWorkspace()
        R, color, radii, _, _, _ = rp.RasterizeGaussiansCUDA(**a, raw_params=flags, sh_adam=sh_adam, workspace=ws)
        return R, color, radii, ws, rp.lastForwardOnly()
    finally:
        rp._LIB_OVERRIDE = prev


def check_parity(lib_path, dev, cl, cam, bg, flags, **kw):
    """The forward-only image, radii and instance count equal the training forward's bit for bit, and each call asks for
    exactly the sizes gsr_binning_bytes_for / gsr_image_bytes_for name.  Returns (R, image, radii) of the training call."""
    lib = capi.load(lib_path)
    a = inputs(cl, cam, bg, dev, **kw)
    R0, c0, r0, ws0, fo0 = render(lib_path, a, flags)
    R1, c1, r1, ws1, fo1 = render(lib_path, a, flags | FORWARD_ONLY)
    assert (fo0, fo1) == (0, 1)
    assert R0 == R1
    assert torch.equal(c0, c1), "forward-only image differs"
    assert torch.equal(r0, r1), "forward-only radii differ"
    for ws, f in ((ws0, flags), (ws1, flags | FORWARD_ONLY)):
        assert ws.requested[2] == lib.gsr_image_bytes_for(cam.W, cam.H, f)
        if R0:
            assert ws.requested[1] == lib.gsr_binning_bytes_for(R0, f)
    assert lib.gsr_binning_bytes_for(R0, flags) == lib.gsr_binning_bytes(R0)
    assert lib.gsr_image_bytes_for(cam.W, cam.H, flags) == lib.gsr_image_bytes(cam.W, cam.H)
    if R0:
        assert ws1.requested[1] < ws0.requested[1] and ws1.requested[2] < ws0.requested[2]
    return R0, c0, r0


def check_sizes(lib):
    """The forward-only layouts against the training ones, from the size functions alone"""
    for R in (0, 1, 1000, 1 << 20, 3_000_000, 6_200_000):
        assert lib.gsr_binning_bytes_for(R, 0) == lib.gsr_binning_bytes(R)
        assert lib.gsr_binning_bytes_for(R, 64 | 8) == lib.gsr_binning_bytes(R)
        assert lib.gsr_binning_bytes_for(R, FORWARD_ONLY) <= lib.gsr_binning_bytes(R)
        assert lib.gsr_binning_bytes_for(R, FORWARD_ONLY) >= 16 * R
        if R >= 1 << 20:
            assert lib.gsr_binning_bytes_for(R, FORWARD_ONLY) <= 0.35 * lib.gsr_binning_bytes(R), R
    for W, H in ((16, 16), (640, 480), (1920, 1080)):
        T = ((W + 15) // 16) * ((H + 15) // 16)
        assert lib.gsr_image_bytes_for(W, H, 0) == lib.gsr_image_bytes(W, H)
        assert 8 * T <= lib.gsr_image_bytes_for(W, H, FORWARD_ONLY) < 8 * T + 1024
        assert lib.gsr_image_bytes(W, H) >= 8 * W * H


def check_backward_guard(lib_path, dev, cl, cam, bg):
    """gsr_backward refuses the buffers of a forward-only call; after a training forward on the same buffers it runs.  A
    forward-only call with a non-lazy sh_adam is refused."""
    a = inputs(cl, cam, bg, dev)
    rp._LIB_OVERRIDE = lib_path
    try:
        ws = rp.RasterWorkspace()
        dpix = torch.ones((3, cam.H, cam.W), device=dev)

        def backward(R, radii):
            geom, binning, img = ws.bufs
            return rp.RasterizeGaussiansBackwardCUDA(a["background"], a["means3D"], radii, a["colors"], a["scales"], a["rotations"],
                                                     1.0, a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], cam.tanfovx,
                                                     cam.tanfovy, dpix, a["sh"], 3, a["campos"], geom, R, binning, img)
        # a training forward first: the workspace's buffers then have the training sizes and are reused as they are
        R, _, radii, _, _, _ = rp.RasterizeGaussiansCUDA(**a, workspace=ws)
        R, _, radii, _, _, _ = rp.RasterizeGaussiansCUDA(**a, raw_params=FORWARD_ONLY, workspace=ws)
        try:
            backward(R, radii)
        except capi.GsrError as e:
            assert e.status == -1
        else:
            raise AssertionError("gsr_backward accepted the buffers of a forward-only pass")
        R, _, radii, _, _, _ = rp.RasterizeGaussiansCUDA(**a, workspace=ws)
        g = backward(R, radii)
        assert torch.isfinite(g[3]).all() and g[3].abs().sum() > 0
        adam = dict(exp_avg=torch.zeros_like(a["sh"]), exp_avg_sq=torch.zeros_like(a["sh"]), lr=1e-3, lr_tail=1e-4, beta1=0.9,
                    beta2=0.999, eps=1e-15, step=1)
        lib = capi.load(lib_path)
        args = capi.ForwardArgs()
        adam_s, keep = capi.make_sh_adam(a["sh"], adam)
        args.P, args.D, args.M, args.width, args.height = a["means3D"].shape[0], 3, 16, cam.W, cam.H
        for name, t in (("background", a["background"]), ("means3D", a["means3D"]), ("shs", a["sh"]), ("opacities", a["opacity"]),
                        ("scales", a["scales"]), ("rotations", a["rotations"]), ("viewmatrix", a["viewmatrix"]),
                        ("projmatrix", a["projmatrix"]), ("cam_pos", a["campos"])):
            setattr(args, name, t.data_ptr())
        out = torch.empty((3, cam.H, cam.W), device=dev)
        args.out_color = out.data_ptr()
        args.scale_modifier, args.tan_fovx, args.tan_fovy = 1.0, cam.tanfovx, cam.tanfovy
        args.raw_params = FORWARD_ONLY
        import ctypes as C
        args.sh_adam = C.cast(C.pointer(adam_s), C.c_void_p)
        n = C.c_int(0)
        cbs = [ws.taker(i, dev) for i in range(3)]
        st = lib.gsr_forward(C.byref(args), cbs[0], None, cbs[1], None, cbs[2], None, rp._stream_ptr(a["means3D"]), C.byref(n))
        assert st == -1, st
    finally:
        rp._LIB_OVERRIDE = None


def check_lazy_read_only(lib_path, dev, cl, cams, bg, window=4, steps=7, seed=0):
    """Lazily stepped SH rows that lag by 1 .. window - 1 steps: the forward-only image equals the training image after a flush,
    bit for bit, and the forward-only call leaves param, both moments and row_step unchanged, byte for byte."""
    rp._LIB_OVERRIDE = lib_path
    try:
        rng = np.random.default_rng(seed)
        P = cl.xyz.shape[0]
        sh = _t(cl.get_features().copy(), dev).clone()
        m = _t((0.01 * rng.standard_normal(sh.shape)).astype(np.float32), dev)
        v = _t((1e-4 * rng.random(sh.shape)).astype(np.float32), dev)
        S = 9   # steps the tensor has taken
        lrs = [0.0025 * (1.0 + 0.1 * k) for k in range(window)]   # lrs[k] = the learning rate of step S - k
        # lags 0 .. window - 1, spread over the rows
        row_step = torch.from_numpy((S - (np.arange(P) % window)).astype(np.int32)).to(dev)
        base = dict(exp_avg=m, exp_avg_sq=v, beta1=0.9, beta2=0.999, eps=1e-15, window=window)
        view_adam = dict(base, lr=lrs[0], lr_tail=lrs[0] / 20, step=S + 1, row_step=row_step, lr_past=lrs,
                         lr_tail_past=[x / 20 for x in lrs])
        a = inputs(cl, cams[0], bg, dev, sh=sh)
        before = [t.clone() for t in (sh, m, v, row_step)]
        images = []
        for cam in cams:
            a = inputs(cl, cam, bg, dev, sh=sh)
            R, color, radii, _, fo = render(lib_path, a, FORWARD_ONLY, sh_adam=view_adam)
            assert fo == 1
            if dev.type != "cpu":
                torch.cuda.synchronize()
            for x, y in zip((sh, m, v, row_step), before):
                assert torch.equal(x, y), "a forward-only render wrote the lazy Adam state"
            images.append((color.clone(), radii.clone(), (radii > 0) & (row_step < S)))
        assert any(bool(lag_vis.any()) for _, _, lag_vis in images), "no lagging row was visible"
        # the training forward after a flush
        rp.shAdamFlush(sh, dict(base, lr=lrs[0], lr_tail=lrs[0] / 20, step=S, row_step=row_step, lr_past=lrs[1:],
                                lr_tail_past=[x / 20 for x in lrs[1:]]))
        assert bool((row_step == S).all())
        assert not torch.equal(sh, before[0])   # (the flush did move the lagging rows)
        for cam, (color, radii, _) in zip(cams, images):
            a = inputs(cl, cam, bg, dev, sh=sh)
            R, c_train, r_train, _, fo = render(lib_path, a, 0)
            assert fo == 0
            assert torch.equal(color, c_train), "forward-only lazy image differs from the flushed training image"
            assert torch.equal(radii, r_train)
    finally:
        rp._LIB_OVERRIDE = None


def lazy_scene(P, W, H, seed):
    """a cloud and keyframes that look in different directions (the culled sets change: SH rows fall behind)"""
    from photo_slam_amd import scene
    cl = scene.make_cloud(P, W, H, 40.0, 40.0, seed=seed, scale_k=0.35)
    cams = [scene.make_camera(W, H, 40.0, 40.0, scene.look_rotation(yaw, 0.1 * k), np.array([0.3 * k, 0.0, -0.2 * k]))
            for k, yaw in enumerate((0.0, 0.9, -0.9, 2.2))]
    return cl, cams


def check_host_modes(ops, lib_path, dev, cl, cam, bg):
    """GaussianRasterizer(Ex)::forward of both hosts: under NoGradGuard / torch.no_grad(), with inputs that do not require grad,
    and with forward_only_ set, the image has no grad_fn and the call was forward-only; with grad on and leaves that require grad
    the training path is unchanged.  The image is the same in every mode."""
    from photo_slam_amd.gaussian_rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    lib = capi.load(lib_path)
    a = inputs(cl, cam, bg, dev)
    bgt = _t(bg, dev)

    def leaves(grad):
        return [a[k].clone().requires_grad_(grad) for k in ("means3D", "sh", "opacity", "scales", "rotations")]
    empty = torch.empty(0, device=dev)
    images = []
    # C++ host
    for ex, fo_ext, no_grad, grad, want in ((False, False, False, True, 0), (False, False, True, True, 1), (False, False, False, False, 1),
                                            (True, False, False, True, 0), (True, True, False, True, 1), (True, False, True, True, 1),
                                            (True, False, False, False, 1)):
        m3, sh, op, sc, rot = leaves(grad)
        m2 = torch.zeros_like(m3, requires_grad=grad)
        color, radii = ops.rasterize_gaussians_modes(m3, m2, sh, empty, op, sc, rot, empty, bgt, 1.0, a["viewmatrix"], a["projmatrix"],
                                                     cam.tanfovx, cam.tanfovy, cam.H, cam.W, 3, a["campos"], ex, 0, fo_ext, no_grad)
        assert lib.gsr_last_forward_only() == want, (ex, fo_ext, no_grad, grad)
        assert (color.grad_fn is None) == bool(want), (ex, fo_ext, no_grad, grad)
        images.append(color.detach())
    # Python host
    rp._LIB_OVERRIDE = lib_path
    try:
        for fo_set, no_grad, grad, want in ((False, False, True, 0), (False, True, True, 1), (False, False, False, 1), (True, False, True, 1)):
            s = GaussianRasterizationSettings(cam.H, cam.W, cam.tanfovx, cam.tanfovy, bgt, 1.0, a["viewmatrix"], a["projmatrix"], 3,
                                              a["campos"], False, forward_only_=fo_set)
            m3, sh, op, sc, rot = leaves(grad)
            m2 = torch.zeros_like(m3, requires_grad=grad)
            with torch.set_grad_enabled(not no_grad):
                color, radii = GaussianRasterizer(s)(m3, m2, op, True, False, True, True, False, shs=sh, scales=sc, rotations=rot)
            assert lib.gsr_last_forward_only() == want, (fo_set, no_grad, grad)
            assert (color.grad_fn is None) == bool(want), (fo_set, no_grad, grad)
            images.append(color.detach())
    finally:
        rp._LIB_OVERRIDE = None
    for im in images[1:]:
        assert torch.equal(im, images[0])


def _snapshot_py(g):
    st = g.optimizer_.state[id(g._features)]
    rs = st.get("row_step")
    return [g._features.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), None if rs is None else rs.clone()] + \
        [p.detach().clone() for p in (g.xyz_, g.opacity_, g.scaling_, g.rotation_)]


def run_python_interleaved(lib_path, dev, cl, cams, with_views, iterations=20, window=4):
    """Python host: `iterations` train steps with lazy SH Adam and a densification in the range; with_views: a render_view from
    another pose between every two steps, each checked to leave the model, its moments and its lazy state byte-unchanged (and
    the lazy state alive exactly when it was before).  Returns the final parameters and moments."""
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe, GaussianPipelineParams
    from photo_slam_amd.trainer import TrainStep
    import copy
    rp._LIB_OVERRIDE = lib_path
    try:
        torch.manual_seed(0)
        gts = [torch.rand(3, c.H, c.W).to(dev) for c in cams]
        mask = torch.ones(3, cams[0].H, cams[0].W, device=dev)
        bg = torch.zeros(3, device=dev)
        g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
        opt = GaussianOptimizationParams()
        opt.densify_from_iter_, opt.densification_interval_, opt.opacity_reset_interval_, opt.densify_grad_threshold_ = 1, 7, 1000, 2e-5
        g.trainingSetup(opt)
        ts = TrainStep(g, opt, GaussianPipelineParams(), bg, cameras_extent=float(cl.extent), densify=True, seed=7,
                       lazy_sh_adam_window=window)
        kfs = [GaussianKeyframe.from_camera(c, dev) for c in cams]
        views, lazy_views = 0, 0
        for it in range(iterations):
            ts.trainForOneIteration(kfs[it % 3], gts[it % 3], mask, sync_loss=False)
            if with_views and it % 2 == 1:
                lazy = g.optimizer_.is_lazy(g._features)
                before = _snapshot_py(g)
                image = ts.render_view(kfs[3])
                assert image.grad_fn is None and rp.lastForwardOnly() == 1
                assert g.optimizer_.is_lazy(g._features) == lazy, "a view flushed the lazy rows"
                for x, y in zip(_snapshot_py(g), before):
                    assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), "a view changed the model"
                views += 1
                lazy_views += int(lazy)
        assert ts.last_densify_ is not None   # (a densification inside the range)
        if with_views:
            assert views == iterations // 2 and lazy_views > 0
        params = [p.detach().clone() for p in g.params()]
        return params + [m.clone() for p in g.params() for m in g.optimizer_.moments(p)]
    finally:
        rp._LIB_OVERRIDE = None


def run_cpp_interleaved(ops, dev, cl, cams, with_views, iterations=20, window=4):
    """The same on the C++ host (TrainStep::renderView through trainer_render_view): the lazy rows' step counts are the same
    tensor, with the same content, after every view as before it"""
    import copy
    import math
    from photo_slam_amd.gaussian_model import GaussianModel
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    torch.manual_seed(0)
    gts = [torch.rand(3, c.H, c.W).to(dev) for c in cams]
    mask = torch.ones(3, cams[0].H, cams[0].W, device=dev)
    bg = torch.zeros(3, device=dev)
    g0 = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    h = ops.trainer_create(g0.xyz_.detach(), g0.features_.detach(), g0.opacity_.detach(), g0.scaling_.detach(), g0.rotation_.detach(),
                           3, float(cl.extent), bg)
    try:
        ops.trainer_set_options(h, {"densify": 1.0, "cameras_extent": float(cl.extent), "seed": 7.0, "densify_from_iter": 1.0,
                                    "densification_interval": 7.0, "opacity_reset_interval": 1000.0, "densify_grad_threshold": 2e-5,
                                    "lazy_sh_adam_window": float(window)})
        cam_args = [(t(c.viewmatrix), t(c.projmatrix), t(c.campos), 2 * math.atan(c.tanfovx), 2 * math.atan(c.tanfovy), c.H, c.W)
                    for c in cams]
        lazy_views = 0
        for it in range(iterations):
            ops.trainer_render_and_backward(h, *cam_args[it % 3], gts[it % 3], mask)
            ops.trainer_finish(h)
            if with_views and it % 2 == 1:
                rs0 = ops.trainer_features_row_step(h)
                image = ops.trainer_render_view(h, *cam_args[3])
                rs1 = ops.trainer_features_row_step(h)
                assert image.grad_fn is None and image.shape == (3, cams[3].H, cams[3].W)
                assert rs0.numel() == rs1.numel() and torch.equal(rs0, rs1), "a view flushed or moved the lazy rows"
                lazy_views += int(rs0.numel() > 0)
        if with_views:
            assert lazy_views > 0
        return [x.detach().clone() for x in ops.trainer_params(h)] + [x.clone() for x in ops.trainer_moments(h)]
    finally:
        ops.trainer_destroy(h)


def check_workspace(lib_path, dev, cl, cams, exact=True):
    """A training forward into the trainer's workspace, then render_view, then the backward: the view leaves the training
    workspace byte-unchanged, and the gradients equal those of forward -> backward with no view in between."""
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe, GaussianPipelineParams, GaussianRenderer
    from photo_slam_amd.trainer import TrainStep
    import copy
    rp._LIB_OVERRIDE = lib_path
    try:
        bg = torch.zeros(3, device=dev)
        kfs = [GaussianKeyframe.from_camera(c, dev) for c in cams]
        torch.manual_seed(1)
        w = torch.rand(3, cams[0].H, cams[0].W).to(dev)
        grads = []
        for with_view in (False, True):
            g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
            g.trainingSetup(GaussianOptimizationParams())
            ts = TrainStep(g, GaussianOptimizationParams(), GaussianPipelineParams(), bg)
            image, _, _, _ = GaussianRenderer.render(kfs[0], cams[0].H, cams[0].W, g, ts.pipe_, bg, workspace=ts.workspace_)
            if with_view:
                saved = [b.clone() for b in ts.workspace_.bufs]
                ts.render_view(kfs[1])
                for b, s in zip(ts.workspace_.bufs, saved):
                    assert torch.equal(b, s), "render_view wrote the training workspace"
                assert ts.view_workspace_.bufs[0] is not None
            (image * w).sum().backward()
            grads.append([p.grad.clone() for p in (g.xyz_, g.features_, g.opacity_, g.scaling_, g.rotation_)])
        for a, b in zip(*grads):
            if exact:
                assert torch.equal(a, b)
            else:
                # (the device: two runs of the same backward pass differ in the last bits -- the order of the quad-waves' LDS adds)
                assert float((a - b).abs().sum()) <= 1e-4 * float(b.abs().sum()) + 1e-12
    finally:
        rp._LIB_OVERRIDE = None
