"""The backward blend's pixel mapping at the image edges (blend_bwd.hip: one wave per 16x8 half tile, a lane holds the pixel of the
left quad and the pixel 8 columns to its right).  Image sizes that are not multiples of 16 leave edge tiles where only the left quad
of a half is inside the image (width mod 16 <= 8), where a half is entirely outside (height mod 16 <= 8), and partial quads.  The
whole pipeline is compared with the oracle, on the emulator and (marked gpu) on the device, in both forms of the kernel: views this
small take the one-wave-per-quad form by default, GSR_BWD_HALF_TILES=1 selects the half tiles (read per call, gsr_api.hip)."""
import numpy as np
import pytest
import torch

import parity
from photo_slam_amd import capi, scene

# (P, W, H, fx, seed): W mod 16 / H mod 16 in the comment.  Some thousands of visible Gaussians per case, so that the parity bar's
# 99.99th percentile of the per-row errors is not just the one most fragile row of a tiny image.
EDGE_CASES = [
    (20000, 200, 136, 160.0, 11),   # 8 / 8: the last tile column has its right quads outside, the last tile row its bottom half
    (20000, 189, 125, 150.0, 12),   # 13 / 13: partial quads on both edges
    (20000, 164, 116, 130.0, 13),   # 4 / 4: right quads and bottom half outside, the left quads cut
    (8000, 9, 200, 160.0, 14),      # one tile column, its right quads outside
]


def _check(lib_path, dev, oracle, P, W, H, fx, seed):
    cl = scene.make_cloud(P, W, H, fx, fx, seed=seed, scale_k=0.2)
    cam = cl.cameras[0]
    bg = np.array([0.2, 0.5, 0.1], np.float32)
    dpix = np.random.default_rng(seed).standard_normal((3, H, W)).astype(np.float32)
    ores, ocolor, oradii, ograds = parity.run_oracle(oracle, cl, cam, bg, dL_dpix=dpix)
    assert ores.R > 0
    r = parity.run_backend(lib_path, dev, cl, cam, bg, dL_dpix=dpix, flags=64)
    print(dict(V=int((oradii > 0).sum()), R=ores.R), parity.compare(r, ores, ocolor, oradii, ograds, cam))


FORMS = {"half_tiles": "1", "quads": "0"}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("P,W,H,fx,seed", EDGE_CASES)
def test_half_tile_edges_emulator(emu_lib_path, oracle, monkeypatch, form, P, W, H, fx, seed):
    monkeypatch.setenv("GSR_BWD_HALF_TILES", FORMS[form])
    _check(emu_lib_path, torch.device("cpu"), oracle, P, W, H, fx, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("P,W,H,fx,seed", EDGE_CASES)
def test_half_tile_edges_gpu(oracle, monkeypatch, form, P, W, H, fx, seed):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    monkeypatch.setenv("GSR_BWD_HALF_TILES", FORMS[form])
    assert capi.load().gsr_backend() == b"hip-gfx950"
    _check(None, torch.device("cuda:0"), oracle, P, W, H, fx, seed)
