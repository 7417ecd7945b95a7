"""Synthetic tri-modal batches and closed-form deterministic weights.

``make_batch`` is the seeded recipe of §8d (what ``--synthetic 1`` trains on and what bench.py
measures); ``fill_tensor`` / ``fill_state_dict`` overwrite every float tensor of a state_dict with
``scale * hash(name, i)`` (exact integer hash -> uniform [-1,1)), so that the golden generator (build
container, real reference), the tests (CPU restatement, HIP path) and the benchmark can all rebuild the exact
same 42 M parameters from nothing -- weights are never committed.  tests/golden/filler.py re-exports
this module.  ``make_raw_cxr`` makes decoded-JPEG stand-ins (uint8 arrays of varying size) for the image slots of a
batch, which ``builder/data/cxr_transform.collate_raw_cxr`` packs for the GPU input chain.
"""
import zlib

import numpy as np
import torch


def _hash_uniform(name: str, n: int) -> np.ndarray:
    """Exact integer hash (murmur3 finaliser) of (crc32(name), i) -> float64 in [-1, 1)."""
    seed = np.uint64(zlib.crc32(name.encode()))
    M = np.uint64(0xFFFFFFFF)
    x = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B1) + seed * np.uint64(0x85EBCA6B)) & M
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & M
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & M
    x ^= x >> np.uint64(16)
    return x.astype(np.float64) / 2147483648.0 - 1.0


def fill_tensor(name: str, t: torch.Tensor) -> torch.Tensor:
    """Returns a new fp32 tensor of t's shape (integer tensors are returned unchanged)."""
    if not t.is_floating_point():
        return t.clone()
    n = t.numel()
    w = _hash_uniform(name, n)
    leaf = name.rsplit(".", 1)[-1]
    if leaf == "running_var":
        w = 1.0 + 0.25 * w
    elif leaf == "running_mean":
        w = 0.1 * w
    elif leaf in ("gamma",) or (leaf == "weight" and t.dim() == 1):
        w = 1.0 + 0.1 * w                       # LayerNorm / BatchNorm scales
    elif leaf in ("bias", "beta"):
        w = 0.05 * w
    elif "relative_position_bias_table" in name:
        w = 0.2 * w
    elif "cls_token" in name or name.endswith("bottlenecks") or name.endswith("ie_feat.weight"):
        w = 0.7 * w
    elif name.endswith(".pe"):
        return t.clone()                        # sinusoid buffer: keep as built
    elif t.dim() >= 2:
        fan_in = int(np.prod(t.shape[1:]))
        w = w * (1.7 / np.sqrt(max(fan_in, 1)))
    else:
        w = 0.1 * w
    return torch.from_numpy(w.astype(np.float32)).reshape(t.shape)


def fill_state_dict(sd):
    return {k: fill_tensor(k, v) for k, v in sd.items()}


def make_batch(seed: int, B: int, T: int, *, ragged: bool = True, missing_mode: str = "mixed",
               multiimages: int = 0, txt_tokens: int = 128, img_size: int = 224, n_images: int = 3, vslt_type: str = "TIE",
               n_feat: int = 16):
    """Synthetic tri-modal batch following SURVEY.md §8d (seeded, CPU generator).
    Returns a dict of CPU tensors with the trainer-level (post-unpack) meaning.  ``vslt_type="carryforward"``: ``x`` is the
    loader's [B, 3, T, n_feat] hourly item (T = the window size) -- plane 0 values in [0, 1] with zero rows behind the length,
    planes 1 and 2 (mask, delta: read by no model here) zeros -- and ``input_lengths`` lies in 1..T."""
    if vslt_type not in ("TIE", "carryforward"):
        raise ValueError(f"make_batch: vslt_type is TIE or carryforward, got {vslt_type}")
    g = torch.Generator().manual_seed(seed)
    U = lambda *s: torch.rand(*s, generator=g)
    if vslt_type == "carryforward":
        lens = torch.randint(1, T + 1, (B,), generator=g) if ragged else torch.full((B,), T, dtype=torch.long)
        if ragged:
            lens[0] = T
    elif ragged:
        lens = torch.randint(3, T + 1, (B,), generator=g)
        lens[0] = T
    else:
        lens = torch.full((B,), T, dtype=torch.long)
    x = torch.zeros(B, 3, T, n_feat) if vslt_type == "carryforward" else torch.zeros(B, T, 3)
    for b in range(B):
        n = int(lens[b])
        if vslt_type == "carryforward":
            x[b, 0, :n] = U(n, n_feat)
            continue
        x[b, :n, 0] = torch.sort(-24.0 * U(n))[0]
        x[b, :n, 1] = U(n)
        x[b, :n, 2] = torch.randint(0, 18, (n,), generator=g).float()
    x = x.half().float()                                     # 2_train.py:164 rounding
    age, gen = U(B), torch.randint(0, 2, (B,), generator=g).float()
    if missing_mode == "mixed":
        mnum = torch.multinomial(torch.tensor([0.4, 0.2, 0.2, 0.2]), B, True, generator=g)
        mnum[: min(4, B)] = torch.arange(min(4, B))          # make sure every pattern appears
    elif missing_mode == "none":
        mnum = torch.zeros(B, dtype=torch.long)
    else:
        mnum = torch.full((B,), int(missing_mode), dtype=torch.long)
    txt_missing = (mnum == 1) | (mnum == 3)
    img_missing = (mnum == 2) | (mnum == 3)
    txt_len = torch.randint(1, txt_tokens - 1, (B,), generator=g)
    txt_len[txt_missing] = 0
    txt = torch.randn(B, txt_tokens, 768, generator=g)
    txt = txt * (torch.arange(txt_tokens).view(1, -1, 1) < txt_len.view(-1, 1, 1))
    K = int(n_images) if multiimages else 1     # the reference hard-codes 3 (tri_mbt_vsltcls.py:161-162)
    img = U(B, K, 1, img_size, img_size)
    img_time = (-10.0 * U(B, K)).half().float()
    if multiimages:
        absent = U(B, K) < 0.3
        absent[:, 0] = False
        img_time[absent] = 10.0
        img = img * (~absent).view(B, K, 1, 1, 1)
    img[img_missing] = 0
    img_time[img_missing] = 10.0 if multiimages else -1.0
    if not multiimages:
        img, img_time = img[:, 0], img_time[:, 0]
    txt_time = -torch.randint(3, 101, (B,), generator=g).float()
    y = torch.randint(0, 2, (B,), generator=g)
    missing = torch.stack([torch.zeros(B), img_missing.float(), txt_missing.float()], 1)
    return dict(x=x, age=age, gen=gen, input_lengths=lens, txt=txt, txt_lengths=txt_len, img=img,
                img_time=img_time, txt_time=txt_time, y=y, missing=missing, missing_num=mnum)


def make_tie_patients(seed: int, n_patients: int = 32, events_per_hour: int = 50):
    """Seeded stand-ins for the reference's per-admission pickles (keys ``data``, ``delta``, ``data_in_time``, ``age``,
    ``gender``) and their feature range: 30 to 72 hours each, hours without a measurement (``None``) at both ends and inside,
    present hours without an event, and -- every fourth patient -- ``events_per_hour`` events in every hour, so that a
    24-hour window holds more than 1000 of them.  Returns ``(patients, feature_mins, feature_maxs)``."""
    rng = np.random.default_rng(seed)
    fmin = np.linspace(-1.0, 2.0, 18)
    fmax = fmin + np.linspace(3.0, 40.0, 18)
    patients = []
    for i in range(n_patients):
        H = int(rng.integers(30, 73))
        dense = i % 4 == 0
        present = np.ones(H, bool) if dense else rng.random(H) > 0.25
        if not dense:
            present[:int(rng.integers(0, 3))] = False
            present[H - int(rng.integers(0, 3)):] = False
            present[H // 2] = True
        dit = []
        for h in range(H):
            if not present[h]:
                dit.append(None)
                continue
            n = events_per_hour if dense else int(rng.integers(0, 12))          # 0: a present hour without an event
            t = np.sort(np.round(h + rng.random(n), 4))
            dit.append(np.stack([t, rng.random(n), rng.integers(0, 18, n).astype(np.float64)], axis=1).reshape(n, 3))
        data = fmin + (fmax - fmin) * rng.random((H, 18))
        delta = rng.integers(0, 6, (H, 18)).astype(np.float64)
        patients.append(dict(data=data, delta=delta, data_in_time=dit, age=float(rng.random()), gender="M" if rng.integers(2) else "F"))
    return patients, fmin, fmax


def make_tie_store(seed: int, n_patients: int = 32, events_per_hour: int = 50):
    """builder/data/tie_store.TieEventStore of ``make_tie_patients`` (on the host; ``.to(device)`` uploads it)."""
    from .builder.data.tie_store import TieEventStore
    patients, fmin, fmax = make_tie_patients(seed, n_patients, events_per_hour)
    return TieEventStore.from_patients(patients, fmin, fmax)


def make_report_store(seed: int, n_reports: int = 256, width: int = 768, max_tokens: int = 128):
    """builder/data/report_store.ReportStore of seeded stand-ins for the BioBERT report embeddings (on the host; ``.to(device,
    dtype)`` uploads it): report ``i`` is keyed ``"report i"``, lengths drawn like ``make_batch`` draws its ``txt_lengths``
    (uniform on 1 .. max_tokens - 2), except report 0 with ONE token and report 1 with ``max_tokens``; standard normal values."""
    from .builder.data.report_store import ReportStore
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, max_tokens - 1, (n_reports,), generator=g)
    lens[:2] = torch.tensor([1, max_tokens])[:n_reports]
    return ReportStore.from_mapping({f"report {i}": {"embedding": torch.randn(int(n), width, generator=g).numpy()}
                                     for i, n in enumerate(lens.tolist())}, width, max_tokens)


def make_token_report_store(seed: int, n_reports: int = 256, vocab: int = 30000, max_length: int = 128):
    """builder/data/report_store.TokenReportStore of seeded stand-ins for the reference's ``txtDict`` (on the host; ``.to(device)``
    uploads it): report ``i`` is keyed ``(i, 0)``, lengths uniform on 0 .. 160 -- an empty report, the short branch of
    ``clinical_note_transform`` and the trimmed one (more than ``max_length - 3`` ids) all occur --, ids uniform on ``[0, vocab)``."""
    from .builder.data.report_store import TokenReportStore
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, 161, (n_reports,), generator=g)
    return TokenReportStore.from_mapping({(i, 0): torch.randint(0, vocab, (int(n),), generator=g).tolist()
                                          for i, n in enumerate(lens.tolist())}, vocab, max_length)


RAW_CXR_SIZES = ((256, 311), (311, 256), (256, 256), (300, 256))     # h x w of the stand-ins (MIMIC-CXR-JPG resized to ~256)


def make_raw_cxr(seed: int, img_time: torch.Tensor, sizes=RAW_CXR_SIZES):
    """Seeded uint8 [h, w] images for the slots of ``make_batch``'s ``img_time`` that hold an image (multi-image batches
    [B, K]: time != 10; single-image batches [B]: time != -1).  Returns one ``(images, times)`` pair per sample, present
    images first as the reference's loader lists them (dataset_new.py:2102-2118)."""
    rng = np.random.default_rng(seed)
    multi = img_time.dim() == 2
    t = img_time if multi else img_time.view(-1, 1)
    samples = []
    for b in range(t.shape[0]):
        images, times = [], []
        for j in range(t.shape[1]):
            if float(t[b, j]) == (10.0 if multi else -1.0):
                continue
            h, w = sizes[int(rng.integers(len(sizes)))]
            y, x = np.mgrid[0:h, 0:w]
            a = (70 + 90 * rng.random() + 60 * np.sin(x / (20 + 40 * rng.random())) * np.cos(y / (15 + 30 * rng.random()))
                 + 40 * (x / w) + rng.normal(0, 10, (h, w)))
            images.append(np.clip(a, 0, 255).astype(np.uint8))
            times.append(float(t[b, j]))
        samples.append((images, times))
    return samples


def make_cxr_store(seed: int, n_images: int = 256):
    """A CxrStore (builder/data/cxr_store.py, host half) of ``n_images`` of ``make_raw_cxr``'s images, JPEG-encoded as
    ``--raw-images 2`` encodes them."""
    from .builder.data.cxr_store import CxrStore
    samples = make_raw_cxr(seed, torch.zeros(n_images))
    return CxrStore.from_files([jpeg_encode(ims[0]) for ims, _ in samples], names=[f"synthetic/{i:05d}.jpg" for i in range(n_images)])


def stored_cxr_samples(store, seed: int, img_time: torch.Tensor):
    """``make_raw_cxr``'s ``(images, times)`` pairs with seeded handles of ``store`` in place of the arrays."""
    rng = np.random.default_rng(seed)
    multi = img_time.dim() == 2
    t = img_time if multi else img_time.view(-1, 1)
    absent = 10.0 if multi else -1.0
    samples = []
    for b in range(t.shape[0]):
        times = [float(v) for v in t[b] if float(v) != absent]
        samples.append(([store.image(int(rng.integers(store.n_images))) for _ in times], times))
    return samples


def jpeg_encode(image, quality: int = 75) -> bytes:
    """The uint8 [h, w] image as the bytes of the file ``Image.fromarray(image).save(path, 'JPEG')`` writes: 8-bit greyscale,
    baseline, PIL's defaults (what the reference's preprocessing stores, 1_mimic_cxr_preprocess.py:81-82).  PIL is needed for
    this stand-in only -- the decoder (builder/data/jpeg.py, csrc/jpeg.hip) does not use it.  ``image`` None: only the check."""
    try:
        from PIL import Image
    except ImportError as e:
        raise SystemExit("--raw-images 2 writes its synthetic JPEG files with PIL (Pillow), which is not installed; "
                         "--raw-images 1 feeds the same images decoded") from e
    if image is None:
        return b""
    import io
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, "JPEG", quality=quality)
    return buf.getvalue()
