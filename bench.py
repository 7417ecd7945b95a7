"""Headline benchmark: tri-modal training samples/s (BASELINE.json metric) on N MI355X of one node.

    python bench.py --gpus N --steps K --warmup W

N > 1 without a launcher (WORLD_SIZE unset): this process starts ``python -m torch.distributed.run --nnodes=1
--nproc-per-node N --master-addr 127.0.0.1 ... bench.py <same flags>`` as a CHILD before it makes any GPU call, relays
rank 0's JSON line and exits with the child's status.  Launched by the driver under torch.distributed.run (RANK /
LOCAL_RANK / WORLD_SIZE set), it is one rank.

One "step" = one full optimisation step of TRI_MBT_VSLTCLS through the reference's trainer contract (zero_grad,
forward, BCE, backward, AdamW, scheduler, loss.item()) on one synthetic batch that is already resident in HBM.
Workload = BASELINE.json configs[1]: vslt_img_txt, 6 layers, d_model 256, per-GPU batch 64, TIE-len 1000 (full-length
events -> N_v = 1005), one 224x224 CXR, 128 text tokens, bf16 MFMA build, dropout 0.1 (the reference default),
random-init weights.  Weak scaling: every rank runs its own batch of 64; gradients are all-reduced over RCCL
(ddp.GradReducer; under hipGraph replay the step is cut into 3 graphs and the buckets of one go out beside the next).

Timing: W warm-up steps, then K steps bracketed by barrier + torch.cuda.synchronize(); every step ends in the
reference's loss hand-over (the trainer returns the step's loss as a Python float).  Under hipGraph replay that value leaves the
device right behind the forward pass (GraphedTrainStep.publish_loss / wait_loss), so the host prepares and enqueues step k+1
while step k's backward is still running: a single step's host time is no longer its device time, and ms_per_step is the
bracketed region's wall time / K (MAX over ranks), value = global batch / that; the median of the per-step host times is
reported beside it (ms_per_step_median_host).

A plain run does only what the headline figure needs: set-up, warm-up, the timed steps, the outputs (--dump-outputs DIR)
and the JSON line (metric, value, unit, ms_per_step, the step's host times, graph cache, config).  --full adds what takes
measurements of its own after the timed region, and the JSON line then also carries
  roofline      -- the dominant kernel (key-masked attention forward, vslt stream): algorithmic FLOPs 4*B*H*N^2*64 per
                   launch / launch duration, against the 2.5 PFLOP/s dense bf16 peak.  `achieved` / `frac` are the IN-STEP
                   figure, measured live here: after the timed region the step is re-captured with a stream-ordered time
                   stamp (mtmp_timestamp: HIP events cannot be timed inside a replayed hipGraph) in front of and behind every
                   attention-forward launch of the vital-sign stream, --instep-steps more steps are replayed, and the
                   duration is the mean stamp difference minus the stamp pair's own gap (two stamps back to back in the same
                   step).  `probe_*`: the same kernel on the same tensors, K back-to-back launches between ONE pair of HIP
                   events on an otherwise idle device (no other stream of the step beside it) -- reported beside the in-step
                   figure, never as `frac`.  The rocprofv3 average of the same kernel inside replayed steps is committed under
                   profiles/ and quoted as rocprof_avg_us.
  roofline_more -- the same two measurements for the attention backward and the weight-gradient GEMM of the vslt stream.
  cpu_baseline  -- the CPU oracle (fp32 PyTorch restatement of the reference, golden-pinned) timed on this host's
                   cores: BASELINE.md section 3 protocol (full per-GPU batch when the host has >= 32 GB of RAM, else B = 16
                   scaled linearly; 1 warm-up + 3 timed steps, median), rank 0, N = 1 only.
  parity_bf16_vs_fp32 -- the committed parity of the benchmarked build at this size (profiles/parity_at_benchmark_size.json).

--dump-outputs DIR writes what the last timed step handed back (rank 0), for comparing two builds output for output on
the same seeded inputs: loss.npy (float64, the step's loss), params.npy and grads.npy (float32, the trainable parameters
after the step's AdamW update and the step's gradient, from the flat buffers; a fixed seeded sample of DUMP_MAX_ELEMS
positions when the buffer is larger).
"""
import argparse
import datetime
import json
import math
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (importing torch makes no GPU call)
import torch.distributed as dist  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0       # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
DUMP_MAX_ELEMS = 4 * 2 ** 20    # per dumped flat buffer: params + grads stay under 32 MB of float32

WORKLOADS = {
    # name: (per-GPU batch, TIE-len, layers, multiimages, n_images, ragged, missing mode, description)
    "full": (64, 1000, 6, 0, 1, False, "none",
             "BASELINE configs[1]: vslt_img_txt tri_mbt_vsltcls, 6 layers, d_model 256, batch 64/GPU, TIE-len 1000 "
             "(N_v=1005), 224x224 CXR, 128-tok text"),
    "ragged": (64, 1000, 6, 0, 1, True, "mixed",
               "BASELINE configs[3] shape: configs[1] with len ~ U{3..1000} and mixed missing modalities; roofline flops "
               "count the batch's own lengths"),
    "cfg5": (128, 2000, 12, 1, 4, False, "none",
             "BASELINE configs[4]: multiimages with 4 images per sample (N_i=201), TIE-len 2000 (N_v=2005), 12 layers, "
             "batch 128/GPU"),
}


def make_args(wl, dtype: str, dropout: float, hip_graph: int, graph_stages: int, ddp: bool, pack_rows: int = 1, skip_img: int = 1):
    from medical_tri_modal_pilot_amd.control.config import parse_args
    B, T, L, multi, K = WORKLOADS[wl][:5]
    return parse_args(["--input-types", "vslt_img_txt", "--model", "tri_mbt_vsltcls", "--modality-inclusion",
                       "train-missing_test-missing", "--lr-init", "1e-5", "--output-type", "intubation",
                       "--batch-size", str(B), "--transformer-num-layers", str(L), "--vslt-type", "TIE", "--TIE-len", str(T),
                       "--model-types", "detection", "--imgtxt-time", "1", "--mbt-only-vslt", "1", "--multiimages", str(multi),
                       "--n-images", str(max(K, 1)), "--dropout", str(dropout), "--compute-dtype", dtype,
                       "--hip-graph", str(hip_graph), "--graph-stages", str(graph_stages), "--ddp", str(int(ddp)),
                       "--pack-rows", str(pack_rows), "--skip-missing-images", str(skip_img), "--synthetic", "1"])


def cpu_baseline(wl, shapes, budget_s: float = 300.0):
    """Oracle (port of the reference's CPU path) on the workload's own batch: BASELINE.md section 3 -- the full per-GPU batch
    when the host has >= 32 GB of RAM (config 2 needs ~22 GB), else B = 16 with linear scaling stated; 1 warm-up + 3 timed
    steps, median (the protocol's three whenever a step takes under 100 s: ~50 s on the GPU boxes' 128 host threads).
    The warm-up step is timed too: if three more would not fit `budget_s` (slow hosts; the driver's bench run
    has ~10 minutes), fewer steps are timed and the sample says so."""
    from medical_tri_modal_pilot_amd import synthetic
    from oracle import tri_mbt_oracle as O
    B, T, L, multi, K = WORKLOADS[wl][:5]
    try:
        ram_gb = os.sysconf("SC_PAGE_SIZE") * os.sysconf("SC_PHYS_PAGES") / 2 ** 30
    except (ValueError, OSError):
        ram_gb = 0.0
    sample_b = B if ram_gb >= 32 else 16
    if wl == "cfg5":
        sample_b = 2                                  # the reference formulation needs an 8.2 GB score tensor per layer at B = 128
    torch.manual_seed(0)
    sd = {k: synthetic.fill_tensor(k, torch.zeros(s)) for k, s in shapes.items()}
    sd["fusion_transformer.positional_encoding.pe"] = O.sinusoid_table(2500, 256).unsqueeze(0)
    bt = synthetic.make_batch(1234, sample_b, T, ragged=False, missing_mode="none", multiimages=multi, n_images=K)
    tr = O.OracleTrainer(sd, O.Cfg(n_layers=L, dropout=0.1, multiimages=multi), lr_init=1e-5, batch_size=sample_b,
                         iters_per_epoch=100)
    t0 = time.perf_counter()
    tr.step(bt, 1)                                   # warm-up
    warm = time.perf_counter() - t0
    timed = max(1, min(3, int(budget_s // max(warm, 1e-3))))
    ts = []
    for i in range(timed):
        t0 = time.perf_counter()
        tr.step(bt, 2 + i)
        ts.append(time.perf_counter() - t0)
    t = sorted(ts)[len(ts) // 2]
    return {"value": sample_b / t, "unit": "samples/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"oracle full train step (fwd+BCE+bwd+AdamW), fp32, B={sample_b} of the workload's batch of {B} "
                      f"(T={T}, L={L}; host RAM {ram_gb:.0f} GB), 1 warm-up ({warm:.1f} s) + {timed} timed, median {t:.2f} s/step"}


def full_report(a, model, flops, flops_dense, instep, probe, n_tok, world):
    """--full: the roofline figures of the in-step and probe measurements, the committed profile figures and the CPU baseline."""
    def roof(kind, kernel_name):
        fl = flops[kind]
        ins = instep.get(kind)
        pr = probe.get(kind, 0.0)
        ms = ins[0] if ins else pr                # in-step when measured, else (fp32 / eager runs) the probe
        tf = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        d = {"bound": "mfma", "kernel": kernel_name, "achieved": tf, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
             "frac": tf / PEAK_BF16_TFLOPS, "flops_per_launch": fl, "dense_flops_per_launch": flops_dense[kind],
             "flops_counted": ("the launch's own lengths: sum over samples of kv_len^2 (packed stream) or N * kv_len (padded); equal "
                               "to the dense figure on the full workload"),
             "timed_in": ("replayed steps, mtmp_timestamp in front of and behind every launch of this kernel on its stream, "
                          "minus the stamp pair's own gap" if ins else "idle-device probe (no in-step measurement in this mode)"),
             "avg_launch_ms": ms, "launches_timed": ins[1] if ins else (a.probe_launches if pr > 0 else 0),
             "timestamp_gap_us": ins[2] if ins else None,
             "probe_avg_launch_ms": pr or None, "probe_frac": (fl / (pr * 1e-3) / 1e12 / PEAK_BF16_TFLOPS) if pr > 0 else None,
             "probe_timed_in": "back-to-back launches on the step's tensors between one HIP event pair, idle device"}
        return d
    # HBM traffic and the in-step rocprofv3 average of the same kernel come from separate rocprofv3 runs of this
    # script (counters / traces cannot be read from inside it); committed under profiles/ with their method
    traffic = traffic_src = rocprof_us = rocprof_src = None
    tpath = os.path.join(ROOT, "profiles", "roofline_traffic.json")
    tj = {}
    if a.dtype == "bf16" and a.workload == "full" and os.path.exists(tpath):
        with open(tpath) as fh:
            tj = json.load(fh)
        traffic, traffic_src = tj.get("traffic_bytes_per_launch"), f"profiles/roofline_traffic.json ({tj.get('round')})"
        rocprof_us, rocprof_src = tj.get("rocprof_avg_us"), tj.get("rocprof_source")
    # the benchmarked build's parity at THIS size (tests/test_gpu_parity.py: test_bf16_build_vs_fp32_build_at_benchmark_sizes,
    # test_config2_full_size_fp32_step_vs_oracle), measured on the GPU by the test suite and committed with the profiles
    parity = None
    ppath = os.path.join(ROOT, "profiles", "parity_at_benchmark_size.json")
    if a.dtype == "bf16" and os.path.exists(ppath):
        with open(ppath) as fh:
            parity = json.load(fh).get({"full": "config2", "ragged": "config2", "cfg5": "cfg5"}[a.workload])
    rf = roof("attn_fwd", f"attn_fwd_kernel<{'bf16' if a.dtype == 'bf16' else 'float'}> (vslt stream, N={n_tok})")
    rf.update(traffic=traffic, traffic_unit="bytes/launch", traffic_source=traffic_src, rocprof_avg_us=rocprof_us,
              rocprof_source=rocprof_src)
    out = {"parity_bf16_vs_fp32": parity, "roofline": rf}
    out["roofline_more"] = [
        roof("attn_bwd", "attn_bwd_dq_kernel + attn_bwd_dkdv_kernel (vslt stream; algorithmic flops = 2.5 x forward)"),
        roof("gemm_tn", "gemm_tn_dma_kernel (vslt-stream QKV weight gradient, M x 768 x 256; its reduction is deferred into "
                        "the layer's mtmp_reduce_batch launch)")]
    for r, key in zip(out["roofline_more"], ("attn_bwd", "gemm_tn")):      # rocprofv3 averages of the committed trace, as above
        r.update((tj.get("more") or {}).get(key) or {})
    out["roofline_more"] = [r for r in out["roofline_more"] if r["avg_launch_ms"] > 0]
    if world == 1 and not a.no_cpu_baseline:
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if v.is_floating_point()}
        out["cpu_baseline"] = cpu_baseline(a.workload, shapes)
    return out


def dump_outputs(out_dir, loss, flat):
    """--dump-outputs: the last timed step's loss, and the flat parameter / gradient buffers (a fixed seeded sample of
    DUMP_MAX_ELEMS positions when larger), as float .npy files."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    n = flat.data.numel()
    idx = None
    if n > DUMP_MAX_ELEMS:
        g = torch.Generator().manual_seed(0)
        idx = torch.randperm(n, generator=g)[:DUMP_MAX_ELEMS].sort().values.to(flat.data.device)
    np.save(os.path.join(out_dir, "loss.npy"), np.array([loss], dtype=np.float64))
    for name, buf in (("params", flat.data), ("grads", flat.grad)):
        v = buf.detach() if idx is None else buf.detach()[idx]
        np.save(os.path.join(out_dir, name + ".npy"), v.float().cpu().numpy())


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure the roofline kernels (in-step stamps, idle-device probe), "
                         "report the committed profile figures and time the CPU oracle baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's loss, parameters and gradients as DIR/<name>.npy (e.g. bench_outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU oracle baseline")
    ap.add_argument("--hip-graph", type=int, default=1, choices=[0, 1])
    ap.add_argument("--graph-stages", type=int, default=0, help="0 = auto (one graph; with more than one rank two, cut behind the first fusion layer)")
    ap.add_argument("--workload", default="full", choices=sorted(WORKLOADS),
                    help="full = BASELINE configs[1] (the headline number); ragged = configs[3] shape; "
                         "cfg5 = configs[4] (K = 4 images, B 128, TIE-len 2000, 12 layers)")
    ap.add_argument("--packed", type=int, default=0, choices=[0, 1],
                    help="feed the vital-sign events as the ragged PackedTieBatch of builder/data (SURVEY 8 f-1)")
    ap.add_argument("--pack-rows", type=int, default=1, choices=[0, 1],
                    help="0: the reference's padded [B, T] layout in the fusion layers (what the ragged workload is compared with)")
    ap.add_argument("--skip-missing-images", type=int, default=1, choices=[0, 1],
                    help="0: a zero image goes through the frozen encoder for samples without one, as in the reference")
    ap.add_argument("--probe-launches", type=int, default=30,
                    help="(--full) back-to-back launches per kernel of the idle-device probe after the timed region (0 = no probe)")
    ap.add_argument("--instep-steps", type=int, default=12,
                    help="(--full) replayed steps with time stamps around the roofline kernels (the in-step duration; 0 = off)")
    ap.add_argument("--force-ddp", action="store_true",
                    help="run the RCCL reducer even with one rank (exercises the N>1 code path on a 1-GPU box)")
    ap.add_argument("--print-loss", action="store_true")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true",
                    help="REHEARSAL of the N > 1 code path on a one-GPU box (not a measurement): every rank uses GPU 0 and the "
                         "collectives go through gloo -- the staged graphs, the merged collectives, the plan check, the broadcast "
                         "and the rank-equality check at the end run exactly as with RCCL")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / rendezvous check without a GPU: every rank joins a gloo group, barriers, and rank 0 "
                         "prints a JSON line")
    return ap.parse_args()


def self_launch(a) -> int:
    """--gpus N > 1 and no launcher environment: run N ranks as children of this (GPU-free) process."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.run(cmd, env=env).returncode


def main():
    a = parse()
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        sys.exit(self_launch(a))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    ddp = world > 1 or a.force_ddp
    if ddp and "MASTER_ADDR" not in os.environ:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29541")
    if a.dry_run:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        t = torch.tensor([float(rank)])
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.barrier()
        if rank == 0:
            print(json.dumps({"dry_run": True, "n_gpus": world, "rccl_ranks": dist.get_world_size(), "max_rank": int(t)}))
        dist.destroy_process_group()
        return
    if a.rehearse_on_one_gpu:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if ddp and a.rehearse_on_one_gpu:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    elif ddp:
        # RCCL prints a version banner on stdout when its communicator comes up: keep stdout for the JSON line
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            # one node: RCCL's bootstrap goes over loopback (the host name of these boxes may not resolve); a rendezvous that does not
            # complete fails after five minutes instead of holding the job for the default half hour
            os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, timeout=datetime.timedelta(seconds=300))
            dist.all_reduce(torch.zeros(1, device=dev))
            torch.cuda.synchronize()
        finally:
            sys.stdout.flush()
            os.dup2(saved_fd, 1)
            os.close(saved_fd)

    from medical_tri_modal_pilot_amd import ops, synthetic
    from medical_tri_modal_pilot_amd.builder.trainer import get_trainer
    from medical_tri_modal_pilot_amd.builder.utils.cosine_annealing_with_warmup_v2 import CosineAnnealingWarmupRestarts
    from medical_tri_modal_pilot_amd.train import _Logger, build_training

    B_PER_GPU, TIE_LEN, LAYERS, multi, n_img, ragged, miss_mode, wl_text = WORKLOADS[a.workload]
    args = make_args(a.workload, a.dtype, a.dropout, a.hip_graph, a.graph_stages, ddp, a.pack_rows, a.skip_missing_images)
    torch.manual_seed(412)
    model, opt, crit = build_training(args, dev, ddp)
    model.train()
    sched = CosineAnnealingWarmupRestarts(opt, first_cycle_steps=args.t_0 * 100, cycle_mult=args.t_mult,
                                          max_lr=args.lr_init * math.sqrt(args.batch_size), min_lr=1e-6,
                                          warmup_steps=args.t_up * 100, gamma=args.gamma)

    bt = synthetic.make_batch(1234 + rank, B_PER_GPU, TIE_LEN, ragged=ragged, missing_mode=miss_mode, multiimages=multi,
                              n_images=n_img)
    d = {k: v.to(dev) for k, v in bt.items() if k != "missing"}
    static = torch.stack([d["gen"], d["age"]], 1)
    x_in = d["x"]
    if a.packed:
        from medical_tri_modal_pilot_amd.builder.data import collate_packed
        x_in = collate_packed([(bt["x"][b, :int(n)].numpy(), static[b].cpu().numpy(), float(bt["txt_time"][b]))
                               for b, n in enumerate(bt["input_lengths"])])
    kw = dict(args=args, x=x_in, static=static, y=d["y"], output_lengths=None, model=model, logger=_Logger(),
              device=dev, scheduler=sched, optimizer=opt, criterion=crit, x_txt=d["txt"], x_img=d["img"],
              imgtxt_time=(d["img_time"], d["txt_time"]), scaler=None, missing=bt["missing"], flow_type="train",
              reports_tokens=None, reports_lengths=None, criterion_aux=(None, None))
    in_len_host = bt["input_lengths"]            # lengths stay on the host like the reference loader's

    # host-side enqueue time: from step start until the trainer blocks in loss.item()
    enq = {"t0": 0.0, "sum": 0.0, "n": 0, "on": False}
    raw_item = torch.Tensor.item

    def timed_item(self):
        if enq["on"] and enq["t0"] > 0:
            enq["sum"] += time.perf_counter() - enq["t0"]
            enq["n"] += 1
            enq["t0"] = 0.0
        return raw_item(self)

    torch.Tensor.item = timed_item
    # graph-mode steps hand their loss over through GraphedTrainStep.wait_loss (no .item()): same stop-watch there
    from medical_tri_modal_pilot_amd import graph as _graph
    raw_wait = _graph.GraphedTrainStep.wait_loss

    def timed_wait(self, *a_, **k_):
        if enq["on"] and enq["t0"] > 0:
            enq["sum"] += time.perf_counter() - enq["t0"]
            enq["n"] += 1
            enq["t0"] = 0.0
        return raw_wait(self, *a_, **k_)

    _graph.GraphedTrainStep.wait_loss = timed_wait

    def step(it):
        enq["t0"] = time.perf_counter()
        return get_trainer(iteration=it, input_lengths=in_len_host, txt_lengths=d["txt_lengths"], **kw)[1]

    for i in range(a.warmup):
        step(i + 1)
    enq["on"] = True
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss, per_step = 0.0, []
    for i in range(a.steps):
        ts = time.perf_counter()
        loss = step(a.warmup + i + 1)            # returns with the step's loss; under graph replay the backward / AdamW may still run
        per_step.append(time.perf_counter() - ts)
        if a.print_loss:
            print(f"step {a.warmup + i + 1} loss {loss:.6f}", file=sys.stderr)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    enq["on"] = False
    torch.Tensor.item = raw_item
    _graph.GraphedTrainStep.wait_loss = raw_wait
    host_ms = 1e3 * enq["sum"] / max(1, enq["n"])
    med = statistics.median(per_step)
    gs = getattr(model, "_mtmp_graph_step", None)
    graphed = gs is not None and gs.replays >= a.steps and not gs.disabled
    n_graphs = 0 if not graphed else max(len(e.get("graphs", [])) for e in gs.entries.values())
    # what the captured graphs hold on to (they cannot be released on this ROCm: graph.py): taken HERE, for the timed steps' cache
    graph_cache = gs.stats() if gs is not None else None
    if graph_cache is not None:
        graph_cache["device_reserved_bytes"] = int(torch.cuda.memory_reserved(dev))
        graph_cache["device_peak_reserved_bytes"] = int(torch.cuda.max_memory_reserved(dev))
    if world > 1:
        t = torch.tensor([dt, med], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt, med = float(t[0]), float(t[1])
    if not math.isfinite(loss):
        raise SystemExit(f"non-finite loss {loss}")
    ranks_agree = None
    if world > 1:
        # data-parallel ranks start from rank 0's parameters and apply the same all-reduced gradients: after the run every rank
        # must hold the SAME parameters, bit for bit (outside the timed region; a violation is a bug in the reducer, not noise)
        flat = opt.flat.data
        cs = torch.stack([flat.double().sum(), flat.double().abs().sum(), flat[::997].double().square().sum()])
        lo, hi = cs.clone(), cs.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        ranks_agree = bool(torch.equal(lo, hi))
        if not ranks_agree:
            raise SystemExit(f"rank {rank}: parameters differ across ranks after {a.warmup + a.steps} steps: {lo.tolist()} vs {hi.tolist()}")
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, loss, opt.flat)

    n_tok = TIE_LEN + 5
    flops_dense = {"attn_fwd": 4.0 * B_PER_GPU * 4 * n_tok * n_tok * 64,
                   "attn_bwd": 10.0 * B_PER_GPU * 4 * n_tok * n_tok * 64,
                   "gemm_tn": 2.0 * B_PER_GPU * n_tok * 768 * 256}
    # The roofline counts the work a launch DOES.  On a ragged batch the attention kernels read keys below kv_len only (always) and,
    # with the packed stream (--pack-rows 1), run no pad query row either; the weight gradient then sees the live rows only.  Pricing
    # those launches at the dense N^2 made the same kernel look 1.5x closer to peak: use the batch's own lengths.
    kv = [min(int(n), TIE_LEN) + 5 for n in in_len_host.tolist()]
    if a.pack_rows:
        flops = {"attn_fwd": 4.0 * 4 * 64 * sum(k * k for k in kv), "attn_bwd": 10.0 * 4 * 64 * sum(k * k for k in kv),
                 "gemm_tn": 2.0 * sum(kv) * 768 * 256}
    else:           # padded layout: every query row runs, against kv_len keys; the weight gradient sees all B * N rows
        flops = {"attn_fwd": 4.0 * 4 * 64 * n_tok * sum(kv), "attn_bwd": 10.0 * 4 * 64 * n_tok * sum(kv),
                 "gemm_tn": flops_dense["gemm_tn"]}
    # ---- in-step duration of the roofline kernels: the step re-captured with time stamps around them (ops.kernel_marks)
    instep = {}
    if a.full and a.instep_steps > 0 and graphed and a.dtype == "bf16":
        ops.marks_enable(dev, 4096, only=("k.", "cal."))
        if gs is not None:
            gs.invalidate()                           # drop the captured graphs: the next steps capture the stamped step
        raw_bce = ops.bce_with_logits

        def bce_cal(*args_, **kws):                   # two stamps back to back inside the step: the stamp pair's own gap
            ops.mark("cal.0.s")
            ops.mark("cal.0.e")
            return raw_bce(*args_, **kws)
        ops.bce_with_logits = bce_cal
        acc = {}
        it0 = a.warmup + a.steps + 1
        for i in range(a.instep_steps + 6):
            ops.marks_new_step()
            step(it0 + i)
            torch.cuda.synchronize()
            if i < 6:                                 # eager warm-up of the new signature + the capture itself
                continue
            mk = ops.marks_read()
            for name, t in mk.items():
                if name.endswith(".s") and name[:-2] + ".e" in mk:
                    acc.setdefault(name[:-2].rsplit(".", 1)[0], []).append(mk[name[:-2] + ".e"] - t)
        ops.bce_with_logits = raw_bce
        ops.marks_disable()
        if gs is not None:
            gs.invalidate()
        gap = statistics.mean(acc.get("cal", [0.0]))
        for kind, key in (("attn_fwd", f"k.attn_fwd.N{n_tok}"), ("attn_bwd", f"k.attn_bwd.N{n_tok}"),
                          ("gemm_tn", f"k.gemm_tn768x256.N{B_PER_GPU * n_tok}")):
            if acc.get(key):
                instep[kind] = (1e-3 * (statistics.mean(acc[key]) - gap), len(acc[key]), gap)
        it0 += a.instep_steps + 6
    else:
        it0 = a.warmup + a.steps + 1
    # ---- idle-device probe: the same kernels on the step's real tensors, back to back between one HIP event pair
    probe = {}
    if a.full and a.probe_launches > 0:
        grabbed = {}
        raw = {"attn_fwd": ops.attn_fwd_grouped, "attn_bwd": ops.attn_bwd_grouped, "gemm_tn": ops.gemm_tn_grouped}

        def grab(name, pred):
            def wrapper(*args_, **kws):
                if name not in grabbed and pred(*args_):
                    grabbed[name] = (args_, kws)
                return raw[name](*args_, **kws)
            return wrapper

        ops.attn_fwd_grouped = grab("attn_fwd", lambda qkvs, *_: qkvs[0].shape[1] == n_tok)
        ops.attn_bwd_grouped = grab("attn_bwd", lambda qkvs, *_: qkvs[0].shape[1] == n_tok)
        ops.gemm_tn_grouped = grab("gemm_tn", lambda dys, xs, *_: dys[0].shape[0] >= B_PER_GPU * TIE_LEN and dys[0].shape[1] == 768)
        args.hip_graph = 0
        step(it0)                                 # one eager step (every rank: it contains the collective)
        args.hip_graph = a.hip_graph
        ops.attn_fwd_grouped, ops.attn_bwd_grouped, ops.gemm_tn_grouped = raw["attn_fwd"], raw["attn_bwd"], raw["gemm_tn"]
        torch.cuda.synchronize()
        for name, (args_, kws) in grabbed.items():
            if name == "gemm_tn":                 # (the deferred-reduction lists are consumed by the step: fresh ones here)
                args_ = (args_[0], args_[1], [None] * len(args_[0]), [[] for _ in args_[0]])
            for _ in range(3):
                raw[name](*args_, **kws)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.probe_launches):
                raw[name](*args_, **kws)
            e1.record()
            torch.cuda.synchronize()
            probe[name] = e0.elapsed_time(e1) / a.probe_launches
        if world > 1:
            dist.barrier()

    if rank == 0:
        out = {
            "metric": "tri-modal training samples/s (fwd+bwd+AdamW step, per-GPU batch %d)" % B_PER_GPU,
            "value": world * B_PER_GPU * a.steps / dt, "unit": "samples/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": 1e3 * dt / a.steps, "ms_per_step_median_host": 1e3 * med,
            "host_enqueue_ms_per_step": host_ms, "hip_graph": bool(graphed), "graphs_per_step": n_graphs,
            "graph_cache": graph_cache,
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": a.dtype, "data": "synthetic (SURVEY 8d recipe), random-init weights",
            "rccl_ranks": dist.get_world_size() if ddp else 1, "ranks_hold_identical_parameters": ranks_agree,
            "rehearsal_on_one_gpu_over_gloo": bool(a.rehearse_on_one_gpu),
            "config": {"workload": wl_text + f", dropout {a.dropout}, mbt-only-vslt 1, imgtxt-time 1"
                                   + (" -- events fed as PackedTieBatch" if a.packed else "")
                                   + ("" if a.pack_rows else " -- padded fusion stack (--pack-rows 0)")
                                   + ("" if a.skip_missing_images else " -- zero images encoded (--skip-missing-images 0)"),
                       "global_batch": world * B_PER_GPU, "parallelism": f"dp{world}", "final_loss": loss},
        }
        if a.full:
            out.update(full_report(a, model, flops, flops_dense, instep, probe, n_tok, world))
        print(json.dumps(out), flush=True)
    if ddp:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
