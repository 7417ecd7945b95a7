"""Token-id reports on the GPU (csrc/token_embed.hip through ops.report_token_ids and ops.TokenEmbedFn): the ids of the
reference's ``--berttype bert`` branch reproduced from a device-resident store (digests of the reference's own ``__getitem__``
output), the embedding lookup bit-equal to ``F.embedding(...).to(dtype)``, its gradient against a float64 sum inside the
worst-case bound of a float32 summation, and model / trainer steps with the kernels against the torch path and the host tensor."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import filler
from medical_tri_modal_pilot_amd.builder.data import ReportStore, TokenReportStore
from tests import token_store_model as M
from tests.report_store_model import rounding_values
from tests.test_gpu_parity import DEV, ROOT, _Logger, _model_sd

pytestmark = pytest.mark.gpu
IN_CHILD = os.environ.get("MTMP_TEST_CHILD") == "1"
F32, BF16 = torch.float32, torch.bfloat16
D = 256


@pytest.fixture(scope="module")
def ops():
    from medical_tri_modal_pilot_amd import ops as _ops
    return _ops


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.detach().cpu().reshape(-1).contiguous().view(torch.uint8).equal(
        b.detach().cpu().reshape(-1).contiguous().view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------- ids gather
@pytest.fixture(scope="module")
def gstore():
    return M.golden_store().to(DEV)


def _edge_store(L):
    lens = (0, 1, 2, 3, 4, 9)
    mapping = {(k, 0): M.golden_ids(50 + k, n) for k, n in enumerate(lens)}
    return TokenReportStore.from_mapping(mapping, max_length=L), TokenReportStore.from_mapping(mapping, max_length=L).to(DEV)


def test_golden_cases(ops, gstore):
    """the 40 cases of the reference's __getitem__ as one batch and as four batches of ten"""
    g = M.golden()
    idx = M.golden_report_idx(gstore)
    host = M.golden_store()
    for lo, hi in [(0, 40), (0, 10), (10, 20), (20, 30), (30, 40)]:
        batch = gstore.plan(idx[lo:hi], g["case_comb"][lo:hi])
        assert batch.txt_lengths.tolist() == g["text_length"][lo:hi].tolist()
        got = ops.report_token_ids(batch, DEV)
        assert got.dtype == torch.int32 and tuple(got.shape) == (hi - lo, 128) and got.is_contiguous()
        assert [M.digest(t) for t in got.float()] == g["sha256"][lo:hi].tolist()
        assert torch.equal(got.cpu().float(), M.plan_ids(batch, host.ids.numpy()))


@pytest.mark.parametrize("L", [3, 5])
def test_edge_lengths(ops, L):
    """max_length 3 (BOS, ONE id, EOS) and 5, reports of 0, 1, 2, 3, 4 and 9 ids: outputs of 18 and 30 elements end in a tail that is
    no 16-byte piece"""
    host, dev = _edge_store(L)
    for idx in ([0, 1, 2, 3, 4, 5], [5], [3, -1, 3], [1, 0, 2, 4, 5, 3, 1]):
        batch = dev.plan(np.asarray(idx, np.int64))
        got = ops.report_token_ids(batch, DEV)
        want = M.plan_ids(batch, host.ids.numpy())
        print(f"report_token_ids[L {L}, reports {idx}]: {got.cpu().tolist()}")
        assert tuple(got.shape) == (len(idx), L) and torch.equal(got.cpu().float(), want)
        assert np.array_equal(got.cpu().numpy(), M.closed_form_ids(batch.first_token, batch.n_tokens, host.ids.numpy(), L))


def test_descriptor_rows_outside_the_store_give_zeros(ops, gstore):
    """through ``tables``: rows the plan would never make -- behind the store's ids, negative -- zero their own sample and leave
    the neighbours exact; the canary rows around ``out=`` keep their value"""
    host = M.golden_store()
    batch = gstore.plan(np.asarray([3, 2, 4, 6, 2, 1], np.int64))
    desc = batch.descriptor()
    desc[1] = torch.tensor([gstore.n_tokens - 2, 5])          # its last three ids lie behind the store
    desc[3] = torch.tensor([0, -4])                           # n < 0
    desc[4] = torch.tensor([-1, 4])
    want = M.plan_ids(batch, host.ids.numpy())
    want[[1, 3, 4]] = 0
    assert np.array_equal(want.numpy(), M.closed_form_ids(desc[:, 0], desc[:, 1], host.ids.numpy(), 128).astype(np.float32))
    big = torch.full((8, 128), -7, dtype=torch.int32, device=DEV)
    out = ops.report_token_ids(batch, DEV, out=big[1:-1], tables=desc.to(DEV))
    assert out.data_ptr() == big[1].data_ptr() and torch.equal(out.cpu().float(), want)
    assert (big[0] == -7).all() and (big[-1] == -7).all()
    desc[4] = torch.tensor([gstore.n_tokens - 200, 200])      # a run that ends exactly at the store's end is in bounds
    ops.report_token_ids(batch, DEV, out=out, tables=desc.to(DEV))
    assert out[4, 0] == 2 and out[4, 127] == 3 and (big[0] == -7).all() and (big[-1] == -7).all()
    with pytest.raises(ValueError, match="out must be a contiguous int32"):
        ops.report_token_ids(batch, DEV, out=torch.empty(6, 128, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="store.to"):
        ops.report_token_ids(host.plan(np.asarray([0, 1])), DEV)


# ---------------------------------------------------------------------------------------------------------------- forward
PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32)]


def _table(V, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(V, D, generator=g)
    r = torch.from_numpy(rounding_values().copy())            # ties both ways, overflow to inf, denormals, +-0
    w[0, :r.numel()] = r
    w[V - 1, -r.numel():] = r
    return w.to(DEV)


def _check_forward(ops, ids, w, tag):
    V = w.shape[0]
    ok = (ids >= 0) & (ids < V)
    for src, dst in PAIRS:
        table = w.to(src)
        want = torch.where(ok.unsqueeze(-1), F.embedding(torch.where(ok, ids, 0).long(), table).to(dst), torch.zeros((), dtype=dst, device=DEV))
        got = ops.token_embed_fwd(ids, table, dst)
        ne = int((got.view(torch.int32 if dst == F32 else torch.int16) != want.view(torch.int32 if dst == F32 else torch.int16)).sum())
        print(f"token_embed_fwd[{tag} {src} -> {dst}]: T {ids.numel()}, V {V}, {int((~ok).sum())} ids out of range: {ne} values differ")
        assert got.dtype == dst and tuple(got.shape) == tuple(ids.shape) + (D,) and _same_bits(got, want)


def test_forward_equals_torch_embedding(ops):
    g = torch.Generator().manual_seed(5)
    _check_forward(ops, torch.randint(0, 7, (15,), generator=g).int().to(DEV), _table(7, 1), "T 15")
    ids = torch.randint(0, 30000, (2, 128), generator=g).int()
    ids[0, :4] = torch.tensor([0, 29999, 0, 29999])
    _check_forward(ops, ids.to(DEV), _table(30000, 2), "T 256")


def test_forward_ids_out_of_range_give_zero_rows(ops):
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(0, 50, (40,), generator=g).int()
    ids[[1, 7, 8, 30, 39]] = torch.tensor([-1, 50, 2 ** 31 - 1, -2 ** 31, 51], dtype=torch.int32)
    _check_forward(ops, ids.to(DEV), _table(50, 3), "out of range")


def test_forward_of_more_than_2_31_bytes(ops):
    """T = 2^21 + 3 float32 rows: the last rows lie past byte 2^31 of the output -- the one size at which a 32-bit byte offset in
    the kernel would show; one launch and three slice comparisons, well under a second"""
    T = (1 << 21) + 3
    w = _table(7, 4)
    ids = (torch.arange(T, device=DEV, dtype=torch.int32) * 5) % 7
    got = ops.token_embed_fwd(ids, w, F32)
    assert got.numel() * 4 > 2 ** 31 and torch.equal(got[-4096:], w[ids[-4096:].long()]) and torch.equal(got[:4096], w[ids[:4096].long()])
    assert torch.equal(got.view(T, D)[:: 1021], w[ids[:: 1021].long()])


def test_token_embed_fn_takes_the_loaders_types(ops):
    """float32 ids (the loader's tensor), int64 and non-contiguous int32 are converted once; the result is F.embedding's"""
    w = torch.nn.Parameter(_table(300, 7))
    ids = torch.randint(0, 300, (4, 128), generator=torch.Generator().manual_seed(8))
    want = F.embedding(ids.to(DEV), w)
    for form in (ids.float().to(DEV), ids.to(DEV), ids.int().to(DEV), ids.int().t().contiguous().to(DEV).t()):
        for dt in (F32, BF16):
            assert _same_bits(ops.TokenEmbedFn.apply(form, w, dt), want.to(dt))


def test_token_embed_fn_backward_outside_the_flat_buffer_and_frozen(ops):
    """a table no optimizer holds gets a dense gradient through autograd (zeros but the touched rows); a frozen one gets none"""
    w = torch.nn.Parameter(_table(300, 9)[:, :].clone())
    ids = torch.randint(0, 300, (2, 40), generator=torch.Generator().manual_seed(10)).int().to(DEV)
    dy = torch.randn(2, 40, D, generator=torch.Generator().manual_seed(12)).to(DEV)
    ops.TokenEmbedFn.apply(ids, w, F32).backward(dy)
    ref, bound, touched = M.embed_grad_reference(ids, dy, 300)
    assert bool(((w.grad.double() - ref).abs() <= bound).all()) and not w.grad[~touched].any()
    x = torch.zeros(1, device=DEV, requires_grad=True)
    frozen = w.detach().clone().requires_grad_(False)
    (ops.TokenEmbedFn.apply(ids, frozen, F32) + x.view(1, 1, 1)).sum().backward()
    assert frozen.grad is None and float(x.grad) == 2 * 40 * D


# --------------------------------------------------------------------------------------------------------------- backward
def _check_backward(ops, ids, V, tag, seed=11):
    """both dy types; twice each, into buffers pre-filled with a pattern between two canary rows"""
    g = torch.Generator().manual_seed(seed)
    T = ids.numel()
    worst = {}
    for dt in (F32, BF16):
        dy = torch.randn(T, D, generator=g).to(dt).to(DEV)                    # (bf16 values are exact in float32)
        ref, bound, touched = M.embed_grad_reference(ids, dy.float(), V)
        runs = []
        for _ in range(2):
            buf = torch.randn(V + 2, D, generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
            prefill = buf.clone()
            dw = ops.token_embed_bwd(ids, dy, buf[1:-1])
            assert dw.data_ptr() == buf[1].data_ptr()
            assert _same_bits(buf[0], prefill[0]) and _same_bits(buf[-1], prefill[-1])                 # canaries
            assert _same_bits(buf[1:-1][~touched], prefill[1:-1][~touched])                              # rows without a token
            runs.append(buf)
        err = (runs[0][1:-1].double() - ref).abs()
        over = int((err > bound)[touched].sum())
        ratio = float((err[touched] / bound[touched].clamp_min(1e-300)).max()) if bool(touched.any()) else 0.0
        counts = torch.bincount(ids[(ids >= 0) & (ids < V)].long(), minlength=1)
        worst[dt] = ratio
        print(f"token_embed_bwd[{tag}, dy {dt}]: T {T}, V {V}, {int(touched.sum())} rows touched, longest list {int(counts.max())}: "
              f"max |err| / bound {ratio:.3g}, {over} elements over the bound")
        assert over == 0
        assert _same_bits(runs[0], runs[1])                                                              # no order is left to chance
    return worst


def test_backward_lists_of_every_kind(ops):
    C = ops.token_embed_chunk()
    g = torch.Generator().manual_seed(21)
    dev = lambda t: t.int().to(DEV)
    _check_backward(ops, dev(torch.tensor([3])), 7, "T 1")
    _check_backward(ops, dev(torch.full((512,), 13)), 50, "T 512, one id")
    _check_backward(ops, dev(torch.randint(0, 50, (1000,), generator=g)), 50, "T 1000 over V 50")
    _check_backward(ops, dev(torch.randperm(30000, generator=g)[:777]), 30000, "all distinct")
    lists = torch.cat([torch.full((C - 1,), 5), torch.full((C,), 6), torch.full((C + 1,), 31), torch.full((2 * C + 1,), 32),
                       torch.full((3,), 49)])
    _check_backward(ops, dev(lists[torch.randperm(lists.numel(), generator=g)]), 50, f"lists of C-1, C, C+1, 2C+1 (C {C})")
    mixed = torch.randint(0, 50, (600,), generator=g)
    mixed[torch.randperm(600, generator=g)[:90]] = torch.tensor([-1, 50, 2 ** 31 - 1, -2 ** 31, 30000, 51]).repeat(15)
    _check_backward(ops, dev(mixed), 50, "out of range mixed in")
    _check_backward(ops, dev(torch.tensor([-1, 7, 7, -5])), 7, "nothing in range")


def test_backward_of_a_batch_of_pad(ops):
    """T 8192, all id 0 (128 chunks of one list), and a batch shaped like the loader's: a third pad, B BOS and B EOS rows"""
    _check_backward(ops, torch.zeros(8192, dtype=torch.int32, device=DEV), 30000, "T 8192, all id 0")
    host = M.golden_store()
    idx = np.asarray([0, 1, 2, 3, 4, 5, 6, -1] * 8, np.int64)
    b = host.plan(idx)
    ids = torch.from_numpy(M.closed_form_ids(b.first_token, b.n_tokens, host.ids.numpy(), 128))
    _check_backward(ops, ids.to(DEV), 30000, "64 golden reports")


# -------------------------------------------------------------------------------------------------- the model and the trainer
LENGTHS = (0, 1, 37, 200)                                     # a missing report, the short branch twice, the trimmed one


def _token_stores():
    mapping = {(k, 0): M.golden_ids(100 + k, n) for k, n in enumerate(LENGTHS)}
    return TokenReportStore.from_mapping(mapping), TokenReportStore.from_mapping(mapping).to(DEV)


def _bert_model(dtype, **over):
    """TRI_MBT_VSLTCLS as tests/test_gpu_parity._product_model builds it, with --berttype bert: 2 layers, closed-form weights"""
    from medical_tri_modal_pilot_amd.control.config import parse_args
    from medical_tri_modal_pilot_amd.builder.models import get_model
    a = parse_args(["--input-types", "vslt_img_txt", "--model", "tri_mbt_vsltcls", "--modality-inclusion",
                    "train-missing_test-missing", "--lr-init", "1e-5", "--batch-size", "4", "--transformer-num-layers", "2",
                    "--imgtxt-time", "1", "--mbt-only-vslt", "1", "--multiimages", "0", "--dropout", "0.0", "--compute-dtype", dtype,
                    "--berttype", "bert"])
    a.device = torch.device(DEV)
    for k, v in over.items():
        setattr(a, k, v)
    model = get_model(a)(a)
    sd = {k: v for k, v in _model_sd(2).items() if not k.startswith("txt_embedding.")}     # (the reference shapes are biobert's Linear)
    model.load_state_dict(sd, strict=False)
    with torch.no_grad():
        model.txt_embedding.weight.copy_(filler.fill_tensor("txt_embedding.weight", torch.zeros(30000, D)))
    return a, model.to(DEV)


def _batch(plan):
    bt = filler.make_batch(4321, 4, 64, missing_mode="none")
    bt["missing"] = torch.stack([bt["missing"][:, 0], bt["missing"][:, 1], plan.missing], 1)
    return bt


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_model_step_with_and_without_the_kernels(ops, dtype, monkeypatch):
    """one forward / backward of TRI_MBT_VSLTCLS (B 4, 2 layers, TIE-len 64) on the same batch with tuning.HIP_TOKEN_EMBED on and
    off: the loss and every gradient but the table's bit-equal, the table's gradient inside the summation bound of the dy a
    tensor hook captured, rows without a token exactly zero"""
    from medical_tri_modal_pilot_amd import tuning
    from medical_tri_modal_pilot_amd.builder.trainer import missing_to_num
    from medical_tri_modal_pilot_amd.optim import FusedAdamW
    host, dev = _token_stores()
    plan = dev.plan(np.asarray([0, 1, 2, 3]))
    ids = ops.report_token_ids(plan, DEV)
    bt = _batch(plan)
    args, model = _bert_model(dtype, hip_graph=0, TIE_len=64)
    model.train()
    model.img_encoder.eval()
    opt = FusedAdamW(model.hot_parameters(), lr=1e-6, weight_decay=1e-6)
    flat = opt.flat
    ti = flat.index_of[id(model.txt_embedding.weight)]
    mnum, _ = missing_to_num(bt["missing"])
    tmax = int(bt["input_lengths"].max())
    dv = lambda t: t.to(DEV)
    grabbed = {}
    real = ops.TokenEmbedFn

    class Hooked:                                             # the kernels' output with a tensor hook on it
        @staticmethod
        def apply(*a):
            y = real.apply(*a)
            y.register_hook(lambda gr: grabbed.__setitem__("on", gr.detach().clone()))
            return y
    monkeypatch.setattr(ops, "TokenEmbedFn", Hooked)

    def grab_off(mod, inp, out):                              # (returns None: a forward hook's return value replaces the output)
        out.register_hook(lambda gr: grabbed.__setitem__("off", gr.detach().clone()))
    handle = model.txt_embedding.register_forward_hook(grab_off)

    def step(on):
        monkeypatch.setattr(tuning, "HIP_TOKEN_EMBED", on)
        opt.zero_grad()
        out, _, _ = model(dv(bt["x"][:, :tmax]), None, None, None, None, dv(bt["age"]), dv(bt["gen"]), dv(bt["input_lengths"].clone()),
                          ids, dv(plan.key_lengths.clone()), dv(bt["img"]), dv(mnum), None, dv(bt["img_time"]), dv(bt["txt_time"]),
                          "train", None, None)
        loss = F.binary_cross_entropy_with_logits(out.squeeze(), dv(bt["y"].float()))
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), flat.grad.detach().clone()
    loss_on, g_on = step(True)
    loss_off, g_off = step(False)
    handle.remove()
    assert set(grabbed) == {"on", "off"} and math.isfinite(float(loss_on))
    print(f"model step[{dtype}]: loss with the kernels {float(loss_on)!r}, with torch ops {float(loss_off)!r}")
    assert _same_bits(loss_on, loss_off)
    lo, hi = flat.slice_of(ti)
    for i, name in enumerate(flat.names):
        a, b = flat.slice_of(i)
        if i != ti:
            assert _same_bits(g_on[a:b], g_off[a:b]), name
    dy = grabbed["on"].float()
    assert _same_bits(dy, grabbed["off"].float())            # (the torch path's hook sits in front of its cast: float32 of the same values)
    ref, bound, touched = M.embed_grad_reference(ids, dy, 30000)
    for tag, gr in (("kernels", g_on), ("torch", g_off)):
        tab = gr[lo:hi].view(30000, D)
        err = (tab.double() - ref).abs()
        print(f"model step[{dtype}] table gradient, {tag}: {int(touched.sum())} rows touched, max |err| / bound "
              f"{float((err[touched] / bound[touched].clamp_min(1e-300)).max()):.3g}")
        if tag == "kernels":
            assert bool((err <= bound).all()) and not tab[~touched].any() and bool(tab[touched].any())
    assert int(touched.sum()) == len(set(ids.flatten().tolist()))


def _steps(bt, x_txt, txt_lengths, hip_graph, dtype):
    """three training steps of TRI_MBT_VSLTCLS --berttype bert (2 layers, TIE-len 64); txt_lengths: one per call"""
    from medical_tri_modal_pilot_amd.builder.trainer import get_trainer
    from medical_tri_modal_pilot_amd.builder.utils.cosine_annealing_with_warmup_v2 import CosineAnnealingWarmupRestarts
    from medical_tri_modal_pilot_amd.optim import FusedAdamW
    args, model = _bert_model(dtype, hip_graph=hip_graph, TIE_len=64)
    model.train()
    model.img_encoder.eval()
    opt = FusedAdamW(model.hot_parameters(), lr=args.lr_init, weight_decay=args.weight_decay)
    sched = CosineAnnealingWarmupRestarts(opt, first_cycle_steps=args.t_0 * 10, cycle_mult=args.t_mult,
                                          max_lr=args.lr_init * math.sqrt(args.batch_size), min_lr=1e-6,
                                          warmup_steps=args.t_up * 10, gamma=args.gamma)
    kw = dict(args=args, x=bt["x"], static=torch.stack([bt["gen"], bt["age"]], 1), y=bt["y"], output_lengths=None, model=model,
              logger=_Logger(), device=torch.device(DEV), scheduler=sched, optimizer=opt, criterion=torch.nn.BCEWithLogitsLoss(),
              x_txt=x_txt, x_img=bt["img"], imgtxt_time=(bt["img_time"], bt["txt_time"]), scaler=None, missing=bt["missing"],
              reports_tokens=None, reports_lengths=None, criterion_aux=(None, None))
    tl = lambda k: None if txt_lengths[k] is None else txt_lengths[k].clone()
    losses = [get_trainer(iteration=it, input_lengths=bt["input_lengths"].clone(), txt_lengths=tl(it - 1), flow_type="train",
                          **kw)[1] for it in (1, 2, 3)]
    torch.cuda.synchronize()
    return losses, opt.flat.data.detach().clone(), args, model, kw


@pytest.mark.parametrize("graph,dtype", [(0, "bf16"), (0, "fp32"), (1, "bf16")])
def test_trainer_steps_on_token_batch_equal_steps_on_host_tensor(graph, dtype):
    """TRI_MBT_VSLTCLS --berttype bert, B 4, 2 layers, TIE-len 64, three steps: the TokenReportBatch through the trainer's
    ops.report_token_ids against the float32 [4, 128] id tensor the reference's loader builds for the same reports (0, 1, 37 and
    200 ids) -- losses and every parameter, bit for bit.  The host run is handed the clamped lengths the plan hands the model;
    the plan run is handed the reference's raw ones (200), which the trainer checks.  The replayed case runs in a process of
    its own, whose graph cache starts empty."""
    if graph == 1 and not IN_CHILD:
        r = subprocess.run([sys.executable, "-m", "pytest", f"{os.path.abspath(__file__)}::"
                            f"test_trainer_steps_on_token_batch_equal_steps_on_host_tensor[{graph}-{dtype}]", "-x", "-q", "-s", "-m",
                            "gpu", "-p", "no:cacheprovider"], env=dict(os.environ, MTMP_TEST_CHILD="1"), cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        print(r.stdout[-3000:], r.stderr[-2000:])
        assert r.returncode == 0 and "1 passed" in r.stdout
        return
    host, dev = _token_stores()
    plan = dev.plan(np.asarray([0, 1, 2, 3]))
    assert plan.txt_lengths.tolist() == [0, 1, 37, 200] and plan.key_lengths.tolist() == [0, 1, 37, 126]
    host_ids = M.plan_ids(plan, host.ids.numpy())
    bt = _batch(plan)
    l_tok, p_tok, args, model, kw = _steps(bt, plan, [None, plan.txt_lengths, None], graph, dtype)
    l_host, p_host, _, model_host, _ = _steps(bt, host_ids, [plan.key_lengths] * 3, graph, dtype)
    print(f"token-store trainer[graph {graph}, {dtype}]: losses plan {l_tok} host tensor {l_host}")
    assert all(math.isfinite(v) for v in l_tok)
    assert [np.float32(v).tobytes() for v in l_tok] == [np.float32(v).tobytes() for v in l_host]
    assert torch.equal(p_tok, p_host)
    if graph == 1:            # both runs replayed steps from a captured graph; none fell back to eager launches
        for m in (model, model_host):
            gs = m._mtmp_graph_step
            print("graph cache:", gs.stats())
            assert not gs.disabled and gs.captures == 1 and gs.replays >= 1 and gs.eager_over_budget == 0
        sig = dict((k, dt) for k, _, dt in model._mtmp_graph_step.capture_log[-1]["signature"][:-1])
        assert sig["x_txt"] == torch.int32
    if graph == 0 and dtype == "bf16":
        from medical_tri_modal_pilot_amd.builder.trainer import get_trainer
        call = lambda **over: get_trainer(**dict(kw, iteration=4, input_lengths=bt["input_lengths"].clone(), flow_type="test", **over))
        with pytest.raises(ValueError, match="txt_lengths differs"):
            call(txt_lengths=plan.key_lengths.clone())       # the clamped lengths are not the reference's textLength
        with pytest.raises(ValueError, match="None or a host tensor"):
            call(txt_lengths=plan.txt_lengths.to(DEV))
        rb = ReportStore.from_mapping({"r": {"embedding": np.ones((3, 768), np.float32)}}).plan(np.asarray([0, 0, 0, 0]))
        with pytest.raises(ValueError, match="--berttype bert reads token ids"):
            call(txt_lengths=None, x_txt=rb)
        args.berttype = "biobert"
        with pytest.raises(ValueError, match="--berttype biobert reads BioBERT token embeddings"):
            call(txt_lengths=None)


def test_training_loop_with_the_token_store_under_hip_graph():
    """train.py --berttype bert --report-store 2 --hip-graph 1 for a handful of iterations at a small size, as the command-line
    tool it is: a process of its own, whose graph cache starts empty"""
    import re
    base = [sys.executable, "-m", "medical_tri_modal_pilot_amd.train", "--input-types", "vslt_img_txt", "--model", "tri_mbt_vsltcls",
            "--modality-inclusion", "train-missing_test-missing", "--lr-init", "1e-5", "--batch-size", "4", "--epochs", "1",
            "--transformer-num-layers", "2", "--vslt-type", "TIE", "--imgtxt-time", "1", "--mbt-only-vslt", "1", "--TIE-len", "128",
            "--synthetic", "1", "--iters-per-epoch", "6", "--report-store", "2", "--hip-graph", "1"]
    r = subprocess.run(base + ["--berttype", "bert"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "token store: 256 reports" in r.stdout
    loss = re.search(r"epoch 1: mean loss ([0-9.eE+-]+|nan|inf)", r.stdout)
    assert loss and math.isfinite(float(loss.group(1)))
    m = re.search(r"hipGraph: (\d+) captures, (\d+) replays, (\d+) eager", r.stdout)
    assert m and int(m.group(1)) >= 1 and int(m.group(2)) >= 1 and int(m.group(3)) == 0
