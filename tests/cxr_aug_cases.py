"""The golden cases of the ``random`` / ``randaug`` image chains (tests/golden/cxr_aug_cases.npz, made by
tests/golden/gen/make_golden_cxr_aug.py) as RawCxrBatch objects with their expected float batches.  Shared by
test_cxr_aug_plan_cpu.py and test_cxr_aug_gpu.py; loaded once."""
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cxr_aug_cases.npz")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def names():
    return [str(n) for n in golden()["names"]]


def samples_of(name):
    g = golden()
    srcs, out, i = [str(s) for s in g[f"{name}.srcs"]], [], 0
    for c in g[f"{name}.counts"]:
        ims = [g[f"src.{s}"] for s in srcs[i:i + int(c)]]
        out.append((ims, [-1.0 - j for j in range(len(ims))]))
        i += int(c)
    return out


def plan_of(name):
    """(ops per image or None for ``random``, crop box per image)"""
    g = golden()
    boxes = [tuple(int(v) for v in b) for b in g[f"{name}.boxes"]]
    if str(g[f"{name}.kind"]) == "random":
        return None, boxes
    ops = [[(str(o), float(m)) for o, m in zip(on, mn)] for on, mn in zip(g[f"{name}.ops"], g[f"{name}.mags"])]
    return ops, boxes


@functools.lru_cache(maxsize=None)
def raw_and_expected(name):
    """(RawCxrBatch on the host, expected float32 batch = PIL's result / 255 with IEEE division); neither is written to."""
    from medical_tri_modal_pilot_amd.builder.data.cxr_transform import CxrRandomTransform, collate_raw_cxr
    g = golden()
    K = int(g[f"{name}.K"])
    ops, boxes = plan_of(name)
    raw = collate_raw_cxr(samples_of(name), CxrRandomTransform(int(g[f"{name}.S"]), str(g[f"{name}.kind"])), K,
                          aug_params=ops, crop_params=boxes)
    crop = torch.from_numpy(g[f"{name}.crop"])                       # [B, max(K, 1), S, S] uint8
    want = (crop.float() / 255.0).unsqueeze(2)                       # [B, per, 1, S, S]
    return raw, (want if K else want[:, 0])
