"""Writes tests/golden/frames_pil.npz: what the real `_process_frame` (Pillow) returns for the seeded frames of
tests/_frames_ref.py, so that the tests of the frame preprocessor do not depend on the Pillow of the machine they run on.
Expected outputs only -- the inputs are regenerated from their seeds.  Re-run:  python tests/golden/gen_frames_golden.py

Every output value is float32(u) / float32(127.5) - float32(1) of a byte u, so the file holds the bytes and, once, the
256 values (read off `_process_frame` itself, on a frame that holds every byte); the generator asserts that this
representation is lossless for every case."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))

from tests import _frames_ref as R  # noqa: E402

CASES = [(h, w, size, p) for h, w, size in R.SHAPES for p in R.PATTERNS] + \
        [(33, 77, 32, "random"), (77, 33, 32, "random"), (100, 100, 32, "col_stripes")]


def key(h, w, size, pattern):
    return f"{h}x{w}_{size}_{pattern}"


def main():
    import PIL
    from PIL import Image
    from lwm_amd.cli.vision_chat import _process_frame
    every = np.arange(256, dtype=np.uint8).repeat(3).reshape(16, 16, 3)
    table = _process_frame(Image.fromarray(every), 16)[..., 0].reshape(256)
    assert table.dtype == np.float32 and len(np.unique(table)) == 256
    out = {"table": table, "pillow": np.array(PIL.__version__)}
    for h, w, size, pattern in CASES:
        frames = R.make_frames(h, w, pattern)
        got = np.stack([_process_frame(Image.fromarray(f), size) for f in frames])
        assert got.dtype == np.float32 and got.shape == (R.T, size, size, 3)
        codes = np.rint((got.astype(np.float64) + 1) * 127.5).astype(np.uint8)
        assert np.array_equal(table[codes], got), (h, w, size, pattern)
        out[key(h, w, size, pattern)] = codes
    path = os.path.join(HERE, "frames_pil.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
