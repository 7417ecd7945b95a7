"""The golden chest X-ray cases (tests/golden/cxr_cases.npz, made by tests/golden/gen/make_golden_cxr.py) as RawCxrBatch
objects with their expected float batches.  Shared by test_cxr_plan_cpu.py and test_cxr_gpu.py; loaded once."""
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cxr_cases.npz")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def names():
    return [str(n) for n in golden()["names"]]


def transform_of(name):
    from medical_tri_modal_pilot_amd.builder.data.cxr_transform import CxrTransform
    g = golden()
    return CxrTransform(int(g[f"{name}.S"]), str(g[f"{name}.kind"]), bool(int(g[f"{name}.train"])))


def samples_of(name):
    g = golden()
    srcs, out, i = [str(s) for s in g[f"{name}.srcs"]], [], 0
    for c in g[f"{name}.counts"]:
        ims = [g[f"src.{s}"] for s in srcs[i:i + int(c)]]
        out.append((ims, [-1.0 - j for j in range(len(ims))]))
        i += int(c)
    return out


def raw_and_expected(name):
    """(RawCxrBatch on the host, expected float32 batch = PIL's crop / 255 with IEEE division)."""
    from medical_tri_modal_pilot_amd.builder.data.cxr_transform import collate_raw_cxr
    g = golden()
    K = int(g[f"{name}.K"])
    params = [tuple(float(v) for v in p) for p in g[f"{name}.params"]]
    raw = collate_raw_cxr(samples_of(name), transform_of(name), K, affine_params=params)
    crop = torch.from_numpy(g[f"{name}.crop"])                       # [B, max(K, 1), S, S] uint8
    want = (crop.float() / 255.0).unsqueeze(2)                       # [B, per, 1, S, S]
    return raw, (want if K else want[:, 0])
