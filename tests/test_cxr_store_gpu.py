"""The image store on the GPU (builder/data/cxr_store.py, csrc/jpeg.hip: mtmp_jpeg_sync_points, mtmp_jpeg_store_entropy): the
sync rows against the plain-Python model's word for word, ops.cxr_store_decode against PIL's own decodes
(tests/golden/jpeg_cases.npz), batches that mix arrays, file bytes and handles through ops.cxr_prepare, a trainer step fed
handles against the same step fed the files' bytes, and a truncated file refused by name.  All comparisons are exact."""
import math

import numpy as np
import pytest
import torch

import filler
from tests import cxr_store_model as M
from tests import jpeg_cases
from tests.test_gpu_parity import DEV, _Logger, _product_model

pytestmark = pytest.mark.gpu
NAMES = jpeg_cases.names()


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def CT():
    from medical_tri_modal_pilot_amd.builder.data import cxr_transform
    return cxr_transform


def _store(bits=None):
    from medical_tri_modal_pilot_amd.builder.data.cxr_store import CxrStore
    return CxrStore.from_files([jpeg_cases.file_of(n) for n in NAMES], bits, NAMES).to(DEV)


@pytest.fixture(scope="module")
def store():
    return _store()


@pytest.mark.parametrize("bits", M.SUBSEQ_BITS)
def test_sync_rows_equal_the_models(bits, store):
    st = store if bits is None else _store(bits)
    want, status = M.golden_sync(bits)
    got = st.d_sync.cpu().numpy()
    assert st.device == torch.device(DEV) and st.streams is None and st.build_ms > 0
    assert got.shape == want.shape == (st.n_sync, 4) and not status.any()
    print(f"sync rows[{bits}]: {int((got != want).any(1).sum())} of {st.n_sync} rows differ from the model's")
    assert np.array_equal(got, want)
    assert torch.equal(st.d_streams.cpu(), torch.from_numpy(M.golden_store(bits).streams))


def test_sync_rows_built_in_several_chunks_are_the_same(monkeypatch):
    """the build launches cut after every 8 KB of streams, 64 sync rows or 40 segments: offsets relative to each chunk"""
    from medical_tri_modal_pilot_amd.builder.data import cxr_store as CS
    monkeypatch.setattr(CS, "CHUNK_BYTES", 8192)
    monkeypatch.setattr(CS, "CHUNK_SYNC_ROWS", 64)
    monkeypatch.setattr(CS, "CHUNK_SEGS", 40)
    st = CS.CxrStore.from_files([jpeg_cases.file_of(n) for n in NAMES], None, NAMES)
    assert 4 <= len(list(st._chunks())) < 13
    st.to(DEV)
    assert np.array_equal(st.d_sync.cpu().numpy(), M.golden_sync(None)[0])


def _check(ops, st, indices, what):
    pixels, sizes = ops.cxr_store_decode(st, indices)
    assert pixels.dtype == torch.uint8 and pixels.is_cuda and pixels.numel() == sum(h * w for h, w in sizes)
    got, o = pixels.cpu().numpy(), 0
    for i, (h, w) in zip(indices, sizes):
        want = jpeg_cases.pixels_of(NAMES[i])
        g = got[o:o + h * w].reshape(h, w)
        o += h * w
        print(f"store decode[{what}, {NAMES[i]}]: {int((g != want).sum())} of {want.size} pixels differ from PIL's decode")
        assert (h, w) == want.shape and np.array_equal(g, want)


@pytest.mark.parametrize("bits", M.SUBSEQ_BITS)
def test_store_decode_equals_pil_in_store_order(ops, store, bits):
    _check(ops, store if bits is None else _store(bits), list(range(len(NAMES))), f"{bits}")


def test_store_decode_equals_pil_shuffled_with_a_repeat_and_alone(ops, store):
    order = np.random.default_rng(5).permutation(len(NAMES)).tolist()
    order.insert(4, order[9])                                   # one index twice
    _check(ops, store, order, "shuffled")
    _check(ops, store, [NAMES.index("1x1")], "alone")


def _mixed_samples(st, K, stored: bool):
    """K = 3: absent slots, an array, a file's bytes, handles; as decoded arrays when not ``stored``"""
    px = lambda n: jpeg_cases.pixels_of(n)
    h = (lambda n: st.image(NAMES.index(n))) if stored else px
    f = jpeg_cases.file_of if stored else px
    rng = np.random.default_rng(77)
    plain = rng.integers(0, 256, (19, 23), dtype=np.uint8)
    if K:
        return [([h("cxr_like"), plain], [-1.0, -2.0]), ([], []), ([f("37x51_q30"), h("rst_blocks8"), h("1x1")], [-3.0, -0.5, 0.0]),
                ([h("smooth_opt")], [-4.0])]
    return [([h("cxr_like")], [-1.0]), ([plain], [-2.0]), ([], []), ([f("37x51_q30")], [-3.0]), ([h("smooth_opt")], [-4.0]),
            ([h("5x3")], [-5.0])]


@pytest.mark.parametrize("K", [0, 3])
@pytest.mark.parametrize("kind", ["resize_affine_crop", "randaug"])
def test_cxr_prepare_on_a_mixed_batch_equals_the_batch_of_arrays(ops, CT, store, kind, K):
    n = 6 if K else 5
    kw = {}
    if kind == "randaug":
        tr = CT.CxrRandomTransform(64, kind)
        aug = [("Rotate", 12.0), ("Brightness", 0.3), ("ShearX", -0.1), ("Equalize", 0.0), ("Sharpness", 0.5), ("Identity", 0.0)]
        kw["aug_params"] = [(aug[i], aug[(i + 1) % 6]) for i in range(n)]
    else:
        tr = CT.CxrTransform(64, kind, True)
        kw["affine_params"] = [(3.0 - i, i, -i, 1.0 + 0.02 * i) for i in range(n)]
    mk = lambda ss: CT.collate_raw_cxr(ss, tr, K, generator=torch.Generator().manual_seed(11), **kw)
    raw, plain = mk(_mixed_samples(store, K, True)), mk(_mixed_samples(store, K, False))
    assert raw.n == plain.n == n and raw.jpeg.n == 1 and raw.stored.n == n - 2 and plain.stored is None and plain.jpeg is None
    assert torch.equal(raw.desc, plain.desc) and raw.params == plain.params
    got, want = ops.cxr_prepare(raw.to(DEV)), ops.cxr_prepare(plain.to(DEV))
    print(f"store chain[{kind}, K {K}]: {int((got != want).sum())} of {want.numel()} values differ")
    assert got.shape == want.shape and torch.equal(got, want) and float(want.max()) > 0.5


def test_cxr_prepare_on_an_all_stored_batch_and_on_one_without_stored_images(ops, CT, store):
    tr = CT.CxrTransform(64, "resize_crop", True)
    names = ["cxr_like", "100x9_q100", "rst_rows1"]
    mk = lambda f: CT.collate_raw_cxr([([f(n)], [-1.0]) for n in names], tr, 0)
    raw = mk(lambda n: store.image(NAMES.index(n)))
    byt, plain = mk(jpeg_cases.file_of), mk(jpeg_cases.pixels_of)
    assert raw.pixels is None and raw.jpeg is None and byt.stored is None and plain.stored is None
    dev = raw.to(DEV)
    assert dev.pixels.is_cuda and dev.pixels.numel() == plain.pixels.numel()
    want = ops.cxr_prepare(plain.to(DEV))
    assert torch.equal(ops.cxr_prepare(dev), want) and torch.equal(ops.cxr_prepare(byt.to(DEV)), want)
    assert torch.equal(dev.pixels.cpu(), plain.pixels)          # every byte of the device-only buffer was written


def _one_step(bt, x_img):
    from medical_tri_modal_pilot_amd.builder.trainer import get_trainer
    from medical_tri_modal_pilot_amd.builder.utils.cosine_annealing_with_warmup_v2 import CosineAnnealingWarmupRestarts
    from medical_tri_modal_pilot_amd.optim import FusedAdamW
    args, model = _product_model(2, 0, "fp32", hip_graph=0, TIE_len=96)
    model.train()
    model.img_encoder.eval()
    opt = FusedAdamW(model.hot_parameters(), lr=args.lr_init, weight_decay=args.weight_decay)
    sched = CosineAnnealingWarmupRestarts(opt, first_cycle_steps=args.t_0 * 10, cycle_mult=args.t_mult,
                                          max_lr=args.lr_init * math.sqrt(args.batch_size), min_lr=1e-6,
                                          warmup_steps=args.t_up * 10, gamma=args.gamma)
    loss = get_trainer(args=args, iteration=1, x=bt["x"], static=torch.stack([bt["gen"], bt["age"]], 1), y=bt["y"],
                       input_lengths=bt["input_lengths"].clone(), output_lengths=None, model=model, logger=_Logger(),
                       device=torch.device(DEV), scheduler=sched, optimizer=opt, criterion=torch.nn.BCEWithLogitsLoss(),
                       x_txt=bt["txt"], x_img=x_img, txt_lengths=bt["txt_lengths"].clone(),
                       imgtxt_time=(bt["img_time"], bt["txt_time"]), scaler=None, missing=bt["missing"], flow_type="train",
                       reports_tokens=None, reports_lengths=None, criterion_aux=(None, None))[1]
    torch.cuda.synchronize()
    return loss, opt.flat.data.detach().clone()


def test_trainer_step_on_stored_handles_equals_step_on_file_bytes(CT, store):
    """TRI_MBT_VSLTCLS, B 4, 2 layers, TIE-len 96, fp32, --hip-graph 0, sample 2 without an image: one missing_trainer step fed
    handles against the same step fed the files' bytes -- the loss and every parameter, bit for bit"""
    bt = filler.make_batch(4321, 4, 96, missing_mode="none")
    bt["missing"][2, 1] = 1.0
    bt["img_time"][2] = -1.0
    names = ("cxr_like", "rst_blocks8", None, "noise_q100")
    tr = CT.CxrTransform(224, "resize_affine_crop", True)
    times = [float(t) for t in bt["img_time"]]
    mk = lambda f: CT.collate_raw_cxr([([f(n)], [t]) if n else ([], []) for n, t in zip(names, times)], tr, 0,
                                      generator=torch.Generator().manual_seed(3))
    raw, byt = mk(lambda n: store.image(NAMES.index(n))), mk(jpeg_cases.file_of)
    assert raw.stored.n == 3 and raw.jpeg is None and raw.pixels is None and byt.jpeg.n == 3 and torch.equal(raw.desc, byt.desc)
    assert torch.equal(raw.img_time, bt["img_time"])
    l_st, p_st = _one_step(bt, raw)
    l_by, p_by = _one_step(bt, byt)
    print(f"store trainer: loss handles {l_st} bytes {l_by}")
    assert math.isfinite(l_st) and np.float32(l_st).tobytes() == np.float32(l_by).tobytes()
    assert torch.equal(p_st, p_by)


def test_truncated_file_is_refused_by_name(ops):
    from medical_tri_modal_pilot_amd.builder.data.cxr_store import CxrStore
    st = CxrStore.from_files([jpeg_cases.file_of("37x51_q30"), jpeg_cases.truncated(), jpeg_cases.file_of("5x3")], None,
                             ["p10/a.jpg", "p10/cut.jpg", "p11/b.jpg"])
    with pytest.raises(ValueError, match=r"1 \(p10/cut\.jpg, status 1\).*truncated or corrupt"):
        st.to(DEV)
    assert st.device.type == "cpu" and st.d_sync is None and st.streams is not None      # it stays a host store
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cxr_store_decode(st, [0])
