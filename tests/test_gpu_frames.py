"""The frame preprocessor on the device: lwm_frames_preprocess_u8 and lwm_amd.frames.process_frames are, bit for bit, the
numpy restatement of Pillow's resize + crop + scale (tests/_frames_ref.py, itself pinned to Pillow's recorded outputs by
tests/test_frames_ref.py); every output element is written and nothing outside; and LWM_FRAMES=hip changes no token."""
import types
import warnings

import numpy as np
import pytest

from tests import _frames_abi as A, _frames_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_restatement(shape):
    """T = 3 different frames per call; output prefilled with NaN between guard bytes, workspace with 0xFF"""
    h, w, size = shape
    for pattern in R.PATTERNS:
        out, rc = A.run_torch(R.make_frames(h, w, pattern), size)
        assert rc == 0, pattern
        assert not np.isnan(out).any(), (pattern, "an output element was not written")
        assert np.array_equal(out, R.expected(h, w, size, pattern)), pattern


def test_equals_recorded_pillow_outputs():
    """straight against what Pillow returned when tests/golden/frames_pil.npz was written"""
    import os
    from tests.golden import gen_frames_golden as G
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames_pil.npz"))
    for h, w, size, pattern in [c for c in G.CASES if c[2] == 32]:
        out, rc = A.run_torch(R.make_frames(h, w, pattern), size)
        assert rc == 0 and np.array_equal(out, golden["table"][golden[G.key(h, w, size, pattern)]]), (h, w, size, pattern)


@pytest.mark.parametrize("misalign", [1, 2, 3])
def test_frames_at_any_byte_alignment(misalign):
    for h, w in ((37, 61), (16, 40)):
        out, rc = A.run_torch(R.make_frames(h, w, "random"), 16, misalign=misalign)
        assert rc == 0 and np.array_equal(out, R.expected(h, w, 16, "random"))


def test_one_pass_alone_from_caller_tables():
    from lwm_amd.frames import resample_tables
    frames = R.make_frames(40, 61, "random")
    full = resample_tables(40, 61, 16)
    f32 = lambda u: u.astype(np.float32) / np.float32(127.5) - np.float32(1)
    out, rc = A.run_torch(frames, 16, tab=full._replace(v_bounds=None, v_coeffs=None, top=7))
    assert rc == 0 and np.array_equal(out, f32(np.clip(R.resample_unclamped(frames[:, 7:23], full.h_bounds, full.h_coeffs, 2), 0, 255)))
    out, rc = A.run_torch(frames, 16, tab=full._replace(h_bounds=None, h_coeffs=None, left=45))
    assert rc == 0 and np.array_equal(out, f32(np.clip(R.resample_unclamped(frames[:, :, 45:61], full.v_bounds, full.v_coeffs, 1), 0, 255)))


def test_the_real_shape():
    """1080p -> 256, T = 2, once: 19 taps, four column strips, 68 row blocks per frame"""
    import torch
    from lwm_amd.frames import process_frames
    frames = np.random.default_rng(5).integers(0, 256, (2, 1080, 1920, 3), dtype=np.uint8)
    frames[1, ::2] = np.where(frames[1, ::2] > 127, 255, 0)
    out = process_frames(frames, 256)
    assert out.shape == (2, 256, 256, 3) and out.dtype == torch.float32 and out.is_cuda
    assert np.array_equal(out.cpu().numpy(), R.process_frames(frames, 256))


def test_process_frames_from_host_and_device():
    import torch
    from lwm_amd.frames import process_frames
    frames = R.make_frames(37, 61, "random")
    want = torch.from_numpy(np.array(R.expected(37, 61, 16, "random")))
    a = process_frames(frames, 16)
    b = process_frames(torch.from_numpy(frames.copy()), 16)
    c = process_frames(torch.from_numpy(frames.copy()).cuda(), 16)
    d = process_frames(torch.from_numpy(frames.copy()).cuda()[:, :, :, :], 16, device=a.device)
    for got in (a, b, c, d):
        assert got.is_cuda and got.dtype == torch.float32 and torch.equal(got.cpu(), want)
    one = process_frames(frames[1], 16)                              # (H,W,3)
    assert one.shape == (1, 16, 16, 3) and torch.equal(one.cpu(), want[1:2])
    strided = torch.from_numpy(frames.copy()).cuda()[::2]            # not contiguous
    assert torch.equal(process_frames(strided, 16).cpu(), want[::2])
    assert process_frames(frames[:0], 16).shape == (0, 16, 16, 3)
    read_only = frames.copy()
    read_only.setflags(write=False)                                  # a memory-mapped clip: no copy, no warning
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert torch.equal(process_frames(read_only, 16).cpu(), want)
    with pytest.raises(ValueError):
        process_frames(frames.astype(np.float32), 16)
    with pytest.raises(ValueError):
        process_frames(torch.from_numpy(frames.copy()).cuda(), 16, device="cpu")


def test_chunked_upload_equals_one_shot(monkeypatch):
    import torch
    from lwm_amd import frames as F
    video = np.concatenate([R.make_frames(37, 61, "random"), R.make_frames(37, 61, "col_stripes")[:2]])     # T = 5
    whole = F.process_frames(video, 16)
    monkeypatch.setattr(F, "CHUNK_BYTES", 2 * 37 * 61 * 3 + 5)       # chunks of 2, 2 and 1 frames
    assert torch.equal(F.process_frames(video, 16), whole)
    assert torch.equal(F.process_frames(torch.from_numpy(video).cuda(), 16), whole)
    monkeypatch.setattr(F, "CHUNK_BYTES", 1)                         # never less than one frame
    assert torch.equal(F.process_frames(video, 16), whole)
    assert torch.equal(whole.cpu(), torch.from_numpy(R.process_frames(video, 16)))


def test_lwm_frames_hip_returns_the_same_tokens(monkeypatch, tmp_path):
    """_read_process_vision on a small .npy of 3 frames and on a .png: the same token list with LWM_FRAMES=hip, =pil and
    unset (the tokeniser sees the same bits)"""
    import torch
    from PIL import Image
    from lwm_amd.cli import vision_chat as VC
    from lwm_amd.vqgan import VQGAN, VQGANConfig, random_params
    cfg = VQGANConfig.get_default_config(dict(resolution=256, channel_mult=(1, 2), num_embeddings=8192))
    vq = VQGAN(params=random_params(cfg, seed=3), config=cfg)
    fake = types.SimpleNamespace(vqgan=vq)
    fake._read_process_vision = types.MethodType(VC.Sampler._read_process_vision, fake)
    video = np.random.default_rng(9).integers(0, 256, (3, 90, 160, 3), dtype=np.uint8)
    npy, png = str(tmp_path / "clip.npy"), str(tmp_path / "picture.png")
    np.save(npy, video)
    Image.fromarray(video[0]).save(png)
    for path in (npy, png):
        monkeypatch.delenv("LWM_FRAMES", raising=False)
        unset = fake._read_process_vision(path, 8)
        assert unset[-1] == 8193 and len(set(unset)) > 20
        monkeypatch.setenv("LWM_FRAMES", "pil")
        assert fake._read_process_vision(path, 8) == unset
        monkeypatch.setenv("LWM_FRAMES", "hip")
        assert fake._read_process_vision(path, 8) == unset
        assert torch.is_tensor(VC.read_frames(path, 8, route="hip")) and VC.read_frames(path, 8, route="hip").is_cuda
    monkeypatch.setenv("LWM_FRAMES", "cuda")
    with pytest.raises(SystemExit):
        fake._read_process_vision(npy, 8)
