"""Frames and expected inputs shared by the uint8-input tests (tests/test_stem_u8_gpu.py, tests/test_engine_u8_input_gpu.py).

A frame is a uint8 (N, H, W, 3) RGB array in which
  * the first 256 pixels of every image (row-major) hold three ramps at different phases, so that every byte value 0..255 appears in
    every channel (frames with fewer than 256 pixels hold as much of the ramps as fits),
  * the last row and the last column are all 255, so that a padded tap normalised as a zero BYTE instead of written as 0.0 changes
    border outputs (normalise(0) != 0 and normalise(255) != 0 for MEAN / STD below),
  * everything else is seeded random bytes.
The expected input is the CPU float32 evaluation of the contract, ((u / 255) - mean) / std: IEEE operations on float32 arrays, no
multiply-add for a compiler to contract."""
import numpy as np

MEAN = [0.485, 0.456, 0.406]
STD = [0.229, 0.224, 0.225]


def frame(n, h, w, seed):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)
    flat = img.reshape(n, h * w, 3)
    k = np.arange(min(256, h * w))
    for c in range(3):
        flat[:, :len(k), c] = ((k + 85 * c + 7 * np.arange(n)[:, None]) % 256).astype(np.uint8)
    img[:, -1, :, :] = 255
    img[:, :, -1, :] = 255
    return img


def expected(img):
    """uint8 (N, H, W, 3) -> float32 (N, 3, H, W), contiguous"""
    f32 = np.float32
    mean32, std32 = np.asarray(MEAN, dtype=f32), np.asarray(STD, dtype=f32)
    x = ((img.astype(f32) / f32(255)) - mean32) / std32
    assert x.dtype == f32
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def covers_every_byte(img):
    return all(len(np.unique(img[i, ..., c])) == 256 for i in range(img.shape[0]) for c in range(3))
