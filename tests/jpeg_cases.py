"""The golden JPEG cases (tests/golden/jpeg_cases.npz, made by tests/golden/gen/make_golden_jpeg.py): file bytes and the array
PIL decodes from them.  Shared by test_jpeg_plan_cpu.py and test_jpeg_gpu.py; loaded once, never written to."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz")
SUBSEQ_BITS = (0, 128, 1024)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def names():
    return [str(n) for n in golden()["names"]]


def file_of(name) -> bytes:
    return golden()[f"file.{name}"].tobytes()


def pixels_of(name) -> np.ndarray:
    return golden()[f"pix.{name}"]


@functools.lru_cache(maxsize=None)
def truncated(name="noise_q100") -> bytes:
    """The file with the second half of its entropy-coded data (and EOI) cut off."""
    from medical_tri_modal_pilot_amd.builder.data.jpeg import parse_jpeg
    data = file_of(name)
    info = parse_jpeg(data)
    return data[:info.ecs_offset + info.ecs_length // 2]


def all_cases_samples(as_jpeg: bool):
    """One image per sample: every case in order, an array image (never a file) between the second and the third."""
    rng = np.random.default_rng(77)
    plain = rng.integers(0, 256, (19, 23), dtype=np.uint8)
    ims = [file_of(n) if as_jpeg else pixels_of(n) for n in names()]
    ims.insert(2, plain)
    return [([im], [-1.0]) for im in ims]
