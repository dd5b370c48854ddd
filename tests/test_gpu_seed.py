"""Seeding Gaussians from an RGB-D frame on the MI355X (GPU twin of test_seed.py; shared checks and their bar: seed_cases.py).  The
sizes are the wave, thread and tile boundaries of the per-pixel kernels, 640 x 411, and the first size past one chunk of the spine scan
(1024 tile totals of 1024 pixels), here with the median.

Measured on the MI355X (every case of this file): written values (xyz relative to the larger of |p_c| and |t|,
scaling, the DC colour and the logit relative to max(1, |value|)) largest relative error 2.95e-7 (xyz, at 1025 x 1024), the emulator
build the same 2.95e-7: bar 1e-5.  Host scene: the first seedFromDepth appends 9911 rows, the second 0, as on the emulator build (the
median's bits differ in the last place, 1060186274 against 1060186270: the two builds' renders do).  The train step after seeding
against the same step after _append_rows: largest parameter difference 2.4e-7 (the backward blend adds with float atomics: two runs
of one program differ in the last bits here; bars rtol 1e-4, atol 1e-6 as tests/test_cpp_host.py).  C++ host against Python host:
identical bits."""
import pytest
import torch

import seed_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device (MI355X)")
    return torch.device("cuda:0")


@pytest.mark.parametrize("W,H", sc.SIZES + [sc.GPU_ONLY_SIZE])
def test_select_and_emit_at_every_size(dev, W, H):
    sc.check_case(None, dev, W, H, seed=W + H)


def test_past_one_chunk_of_the_spine_scan(dev):
    W, H = sc.PAST_ONE_CHUNK
    sc.check_case(None, dev, W, H, seed=1, n_emit=lambda s: s // 3)


def test_median_bits(dev):
    sc.check_median(None, dev)


def test_strides_and_offsets(dev):
    sc.check_strides(None, dev)


def test_thinning(dev):
    sc.check_thinning(None, dev)


def test_corner_values_and_options(dev):
    sc.check_corners(None, dev)


def test_same_bits_on_every_run(dev):
    sc.check_determinism(None, dev)


def test_api_contract(dev):
    sc.check_api_contract(None, dev)


def test_python_host_seeds_what_the_rule_selects(dev):
    sc.check_host_python(None, dev)


def test_python_host_empty_model_caps_and_process_group(dev):
    sc.check_host_empty_and_caps(None, dev)


def test_python_train_step_after_seeding(dev):
    sc.check_host_train_step_after_seeding(None, dev)
