"""The arithmetic of the frame preprocessor, without a device: the numpy restatement (tests/_frames_ref.py) is Pillow's
`_process_frame` bit for bit (against the Pillow installed here, and against outputs recorded in
tests/golden/frames_pil.npz); `lwm_amd.frames.resample_tables` builds the restatement's tables; and the tables stay inside
the bounds the integer kernels rely on."""
import os

import numpy as np
import pytest

from lwm_amd import frames as F
from tests import _frames_ref as R
from tests.golden import gen_frames_golden as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames_pil.npz")
BIG = [(1080, 1920, 256), (2160, 3840, 256), (720, 1280, 256), (1920, 1080, 256)]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_restatement_equals_recorded_pillow_outputs(golden):
    table = golden["table"]
    assert np.array_equal(table, np.arange(256, dtype=np.float32) / np.float32(127.5) - np.float32(1))
    for h, w, size, pattern in G.CASES:
        want = table[golden[G.key(h, w, size, pattern)]]
        got = R.process_frames(R.make_frames(h, w, pattern), size)
        assert got.dtype == np.float32 and np.array_equal(got, want), (h, w, size, pattern)


def test_restatement_equals_the_installed_pillow():
    from PIL import Image
    from lwm_amd.cli.vision_chat import _process_frame
    rng = np.random.default_rng(11)
    shapes = [(h, w, size, p) for h, w, size, p in G.CASES if p in ("random", "col_stripes")]
    for h, w, size, pattern in shapes:
        for f in R.make_frames(h, w, pattern):
            assert np.array_equal(R.process_frame(f, size), _process_frame(Image.fromarray(f), size)), (h, w, size, pattern)
    f = rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)            # the real shape, once
    assert np.array_equal(R.process_frame(f, 256), _process_frame(Image.fromarray(f), 256))


@pytest.mark.parametrize("shape", R.SHAPES + BIG + [(33, 77, 32), (77, 33, 32)], ids=lambda s: "x".join(map(str, s)))
def test_tables_equal_the_restatement_and_keep_the_kernel_bounds(shape):
    h, w, size = shape
    tab = F.resample_tables(h, w, size)
    nw, nh, left, top = R.target(h, w, size)
    assert (tab.nw, tab.nh, tab.left, tab.top) == (nw, nh, left, top)
    assert 0 <= left and left + size <= nw and 0 <= top and top + size <= nh
    assert tab.scale.dtype == np.float32 and tab.scale.shape == (256,)
    assert np.array_equal(tab.scale, np.arange(256, dtype=np.float32) / np.float32(127.5) - np.float32(1))
    for n_in, n_out, first, bounds, coeffs in ((w, nw, left, tab.h_bounds, tab.h_coeffs), (h, nh, top, tab.v_bounds, tab.v_coeffs)):
        if n_in == n_out:
            assert bounds is None and coeffs is None          # a skipped pass is copied, not resampled
            continue
        rb, rk = R.pass_tables(n_in, n_out)
        assert bounds.dtype == np.int32 and coeffs.dtype == np.int32
        assert bounds.shape == (size, 2) and coeffs.shape == (size, rk.shape[1])
        assert np.array_equal(bounds, rb[first:first + size]) and np.array_equal(coeffs, rk[first:first + size])
        # what the kernels rely on, over the WHOLE pass (the restatement's tables, int64)
        assert (rb[:, 0] >= 0).all() and (rb[:, 1] >= 1).all() and (rb[:, 0] + rb[:, 1] <= n_in).all()
        assert (rb[:, 1] <= rk.shape[1]).all()
        assert np.abs(rk).max() < 1 << 23                                # a 24-bit multiply holds pixel * k
        assert (255 * np.abs(rk).sum(1) + (1 << 21) < 1 << 31).all()     # 32-bit accumulators are exact
        for i, (_, taps) in enumerate(rb):
            assert not rk[i, taps:].any()


def test_tap_counts():
    """ksize = 2 * ceil(2 * max(in / out, 1)) + 1"""
    assert R.pass_tables(9, 16)[1].shape[1] == 5                         # upscaling
    assert R.pass_tables(1080, 256)[1].shape[1] == 19
    assert R.pass_tables(2160, 256)[1].shape[1] == 35
    assert R.pass_tables(300, 16)[1].shape[1] == 77
    assert F.resample_tables(1080, 1920, 256).v_coeffs.shape[1] == 19
    assert F.resample_tables(300, 300, 16).h_coeffs.shape[1] == 77


def test_tables_are_cached_and_read_only():
    a, b = F.resample_tables(37, 61, 16), F.resample_tables(37, 61, 16)
    assert a is b
    with pytest.raises(ValueError):
        a.h_coeffs[0, 0] = 1
    with pytest.raises(ValueError):
        F.resample_tables(0, 4, 16)


def test_process_frames_refuses_everything_but_uint8_rgb():
    """checked before a device is needed (and there is no CPU path behind it)"""
    import torch
    ok = np.zeros((2, 8, 8, 3), np.uint8)
    for bad in (ok.astype(np.float32), ok.astype(np.int16), ok[..., :2], ok[..., 0], np.zeros((2, 8, 8, 4), np.uint8),
                np.zeros((1, 2, 8, 8, 3), np.uint8), torch.zeros(2, 8, 8, 3), torch.zeros(8, 8, dtype=torch.uint8), [[1, 2, 3]]):
        with pytest.raises(ValueError):
            F.process_frames(bad, 16)
    with pytest.raises(ValueError):
        F.process_frames(ok, 0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            F.process_frames(ok, 16)


def test_lwm_frames_switch(monkeypatch, tmp_path):
    """unset = `pil`, the host route, exactly as before; anything but hip / pil is refused by name"""
    from lwm_amd.cli import vision_chat as VC
    monkeypatch.delenv("LWM_FRAMES", raising=False)
    assert VC.frames_route() == "pil"
    for v in ("hip", "pil"):
        monkeypatch.setenv("LWM_FRAMES", v)
        assert VC.frames_route() == v
    monkeypatch.setenv("LWM_FRAMES", "gpu")
    with pytest.raises(SystemExit, match="'hip' or 'pil'"):
        VC.frames_route()
    video = R.make_frames(37, 61, "random")
    path = str(tmp_path / "clip.npy")
    np.save(path, video)
    want = np.stack([R.process_frame(f, 256) for f in video])
    assert np.array_equal(VC.read_frames(path, 8), want)                 # the default route is the host's
    assert np.array_equal(VC.read_frames(path, 8, route="pil"), want)
    with pytest.raises(ValueError):
        VC.read_frames(path, 8, route="gpu")
