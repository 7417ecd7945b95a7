"""Training entry for the hot path: the optimiser / scheduler setup and the batch loop of the reference's
``2_train.py`` (:110-124 AdamW + CosineAnnealingWarmupRestarts, :141-200 the loop around ``get_trainer``), with the
build-only flags wired in:

    --synthetic 1     batches from the SURVEY §8d recipe (medical_tri_modal_pilot_amd/synthetic.py); the reference's
                      loaders need private MIMIC data and absent dependencies (out of scope)
    --ddp 1           one process per GPU (launch with ``python -m torch.distributed.run --nproc-per-node N -m
                      medical_tri_modal_pilot_amd.train ...``): RCCL gradient all-reduce through ddp.GradReducer,
                      rank-seeded batches, initial broadcast from rank 0, ``--batch-size`` is per rank
    --fused-adamw 1   optim.FusedAdamW over the flat buffers (0: torch.optim.AdamW(model.parameters()) as in the reference)
    --hip-graph 1     hipGraph replay of zero_grad + forward + backward (needs --fused-adamw 1)
    --raw-images 1    the synthetic batches carry uint8 images of varying size (synthetic.make_raw_cxr) as a RawCxrBatch; the
                      trainer runs the reference loader's equalize / resize / affine / crop chain on the GPU (ops.cxr_prepare);
                      every --image-train-type but resize_larger, RandomResizedCrop (random) and RandAugment (randaug) included
    --raw-images 2    the same images JPEG-encoded (PIL writes them, as the reference's preprocessing does): the batches carry
                      file bytes, and the decoder runs on the GPU in front of that chain (ops.jpeg_decode, csrc/jpeg.hip)
    --raw-images 3    those files in a synthetic device-resident image store (synthetic.make_cxr_store, builder/data/cxr_store.py),
                      built and uploaded once: the batches carry handles, nothing is parsed and no stream or pixel byte is
                      uploaded per batch (ops.jpeg_decode decodes them from the store's sync table)
    --tie-store 1     the vital-sign windows come from a synthetic device-resident event store (synthetic.make_tie_store: None
                      hours at both ends, empty present hours, windows over 1000 events): the loader hands over (patient, hour,
                      length) triples, builder/data/tie_store.py plans them, ops.tie_windows gathers in front of the step
    --vslt-type carryforward
                      the hourly carry-forward table instead of TIE events: [B, 3, window_size, 16] host batches
                      (synthetic.make_batch vslt_type="carryforward"), or with --tie-store 1 the same triples planned by
                      TieEventStore.plan_hourly and gathered by ops.hourly_windows; ops.HourlyEmbedFn embeds the rows
    --report-store 1  the report embeddings come from a synthetic device-resident embedding store (synthetic.make_report_store):
                      the loader hands over one report index per sample, builder/data/report_store.py plans them,
                      ops.report_tokens gathers in front of the step, in the model's compute type
    --val-iters N     a validation pass of N synthetic batches (--val-batch-size, default --batch-size) at the end of every epoch:
                      builder/trainer/validate.py -- the forward replayed from a hipGraph of its own under --hip-graph 1,
                      predictions, targets and the loss sum collected on the device (builder/utils/device_evaluator.py), one
                      64-byte copy per pass.  The batches come from a seed base of their own, the same set every epoch, through
                      the same store flags as training; with --tie-store 1 the windows are those of StoreWindowSweep, in order
                      (every present hour of every patient, as the reference's test data sets enumerate theirs)
    --report-store 2  with --berttype bert: the reports are token ids from a synthetic device-resident id store
                      (synthetic.make_token_report_store: 0 to 160 ids a report, so both trim branches occur);
                      ops.report_token_ids writes the int32 [B, 128] batch, ops.TokenEmbedFn looks the ids up

    python -m medical_tri_modal_pilot_amd.train --input-types vslt_img_txt --model tri_mbt_vsltcls \\
        --modality-inclusion train-missing_test-missing --lr-init 1e-5 --batch-size 64 --epochs 1 \\
        --transformer-num-layers 6 --vslt-type TIE --imgtxt-time 1 --mbt-only-vslt 1 --synthetic 1

What is NOT here: validation / test loops over REAL data (the loop itself is builder/trainer/validate.py, --val-iters runs it on
synthetic batches and tracks the best result like logger.py:115-118), tensorboard logging, checkpoint files on a new best, the
test run of 3_test.py (2_train.py:287-376, SURVEY §2 rows 5, 11 -- harness), validation under --ddp 1.  ``--iters-per-epoch``
replaces ``len(train_loader)`` for synthetic data.
"""
import math
import os
import sys
import time

import torch
import torch.distributed as dist


class _Logger:
    """The two members get_trainer touches (builder/utils/logger.py: log_lr, evaluator.add_batch) + the running loss, and with an
    evaluator (--val-iters: a DeviceEvaluator) the best-result bookkeeping of add_validation_logs (logger.py:91-118)."""

    class _Ev:
        def add_batch(self, *_):
            pass

    def __init__(self, evaluator=None):
        self.evaluator = self._Ev() if evaluator is None else evaluator
        self.loss = 0.0
        self.lr = None
        self.best_auc = getattr(evaluator, "best_auc", 0)
        self.best_iter, self.best_result_so_far = 0, None

    def add_validation_logs(self, step):
        """detection (logger.py:105-118): the anchor is auc + apr; a better one becomes the best result and its iteration"""
        result = self.evaluator.performance_metric()
        auc, apr, _f1 = result
        anchor = auc + apr
        if self.best_auc < anchor:
            self.best_iter, self.best_auc, self.best_result_so_far = step, anchor, list(result)
        return result

    def log_lr(self, lr, _iteration):
        self.lr = lr


VAL_SEED_BASE = 50000017        # the validation batches' seeds: a base of their own, the same set every epoch (epoch 0)


def synthetic_loader(args, n_iters: int, rank: int, epoch: int, tie_store=None, report_store=None, cxr_store=None,
                     batch_size=None, seed_base: int = 0, sweep=None, train: bool = True):
    """n_iters batches of the 12-tuple of 2_train.py:143 (CPU tensors, like the reference's loader output).  The validation
    pass: ``batch_size`` of its own, ``seed_base`` added to every seed, ``sweep`` (a StoreWindowSweep: with an event store the
    windows are its items in order, not drawn), ``train`` False (the evaluation transform of the raw images)."""
    from .synthetic import make_batch
    multi = int(args.multiimages)
    B = int(args.batch_size if batch_size is None else batch_size)
    epoch_seed = seed_base + 7919 * rank + 104729 * epoch
    hourly = args.vslt_type == "carryforward"
    for it in range(n_iters):
        bt = make_batch(1234 + epoch_seed + it, B, int(args.window_size if hourly else args.TIE_len), ragged=True,
                        missing_mode="mixed" if "missing" in args.modality_inclusion else "none", multiimages=multi,
                        img_size=int(args.image_size), n_images=int(getattr(args, "n_images", 3)),
                        vslt_type="carryforward" if hourly else "TIE", n_feat=len(args.vitalsign_labtest))
        static = torch.stack([bt["gen"], bt["age"]], 1)
        if int(getattr(args, "raw_images", 0)) in (1, 2, 3):
            from .builder.data.cxr_transform import collate_raw_cxr, transform_from_args
            from .synthetic import jpeg_encode, make_raw_cxr, stored_cxr_samples
            g = torch.Generator().manual_seed(4241 + epoch_seed + it)
            if int(args.raw_images) == 3:
                samples = stored_cxr_samples(cxr_store, g.initial_seed(), bt["img_time"])
            else:
                samples = make_raw_cxr(g.initial_seed(), bt["img_time"])
            if int(args.raw_images) == 2:
                samples = [([jpeg_encode(im) for im in ims], times) for ims, times in samples]
            raw = collate_raw_cxr(samples, transform_from_args(args, train=train),
                                  int(getattr(args, "n_images", 3)) if multi else 0, generator=g)
            bt["img"], bt["img_time"] = raw, raw.img_time.half().float()
        if tie_store is not None:
            # the vital-sign stream as windows of the device-resident event store: the loader hands over B triples, the plan
            # is host work on the hour-level arrays, the events are gathered in front of the step (ops.tie_windows)
            import random
            from .builder.data.tie_store import StoreWindowDataset
            if sweep is not None:
                triples = [sweep[(it * B + j) % len(sweep)] for j in range(B)]
            else:
                random.seed(977 + epoch_seed + it)
                ds = StoreWindowDataset(tie_store, int(args.window_size))
                triples = [ds[random.randrange(len(ds))] for _ in range(B)]
            if hourly:          # the hourly table of the same windows (ops.hourly_windows gathers it in front of the step)
                wb = tie_store.plan_hourly(triples, int(args.window_size), None, int(args.realtime),
                                           "train-missing" in args.modality_inclusion)
            else:
                wb = tie_store.plan(triples, int(args.TIE_len), int(args.realtime), "train-missing" in args.modality_inclusion)
            bt["x"], static, bt["input_lengths"] = wb, wb.static, wb.input_lengths
            if int(args.realtime) == 1:
                bt["txt_time"] = wb.txt_time
        if report_store is not None:
            # the reports as indices into the device-resident embedding store: the loader hands over B integers, the plan
            # applies the batch's modality combinations (1 and 3 drop the report), the rows are gathered in front of the step
            g = torch.Generator().manual_seed(3373 + epoch_seed + it)
            rb = report_store.plan(torch.randint(0, report_store.n_reports, (B,), generator=g).numpy(),
                                   bt["missing_num"].numpy())
            bt["txt"], bt["txt_lengths"] = rb, rb.txt_lengths
            bt["missing"] = torch.stack([bt["missing"][:, 0], bt["missing"][:, 1], rb.missing], 1)
        yield (bt["x"], static, bt["y"], bt["input_lengths"], bt["img"], bt["img_time"], bt["txt"], bt["txt_lengths"],
               bt["txt_time"], bt["missing"], None, None)


def build_training(args, device, ddp: bool):
    """model, optimizer, criterion exactly as 2_train.py:76-83,110 builds them (plus the flat-buffer AdamW / reducer)."""
    from .builder.models import get_model
    from .optim import FusedAdamW
    args.device = device
    model = get_model(args)(args).to(device)
    if ddp:
        from .ddp import broadcast_module_state
        broadcast_module_state(model, 0)
    if int(args.fused_adamw) == 1 and hasattr(model, "hot_parameters"):
        opt = FusedAdamW(model.hot_parameters(), lr=args.lr_init, weight_decay=args.weight_decay,
                         reference_params=list(model.parameters()))
        if ddp:
            from .ddp import GradReducer
            opt.reducer = GradReducer(opt.flat)
            opt.grad_scale = 1.0 / dist.get_world_size()
    else:
        if ddp:
            raise SystemExit("--ddp 1 needs --fused-adamw 1 (the reducer works on the flat gradient buffer)")
        opt = torch.optim.AdamW(model.parameters(), lr=args.lr_init, weight_decay=args.weight_decay)
    return model, opt, torch.nn.BCEWithLogitsLoss(reduction="mean")


def main(argv=None):
    from .control.config import build_parser
    from .builder.trainer import get_trainer
    from .builder.utils.cosine_annealing_with_warmup_v2 import CosineAnnealingWarmupRestarts
    parser = build_parser()
    parser.add_argument("--iters-per-epoch", type=int, default=100, help="len(train_loader) for synthetic data")
    parser.add_argument("--raw-images", type=int, default=0, choices=[0, 1, 2, 3],
                        help="1: synthetic batches carry uint8 images; the transform chain runs on the GPU (ops.cxr_prepare); "
                             "2: they carry JPEG file bytes, decoded on the GPU in front of it (needs PIL to write the files); "
                             "3: they carry handles of a device-resident store of those files (builder/data/cxr_store.py)")
    parser.add_argument("--tie-store", type=int, default=0, choices=[0, 1],
                        help="1: the vital-sign windows come from a synthetic device-resident event store "
                             "(builder/data/tie_store.py); the loader hands over (patient, hour, length) triples")
    parser.add_argument("--report-store", type=int, default=0, choices=[0, 1, 2],
                        help="1: the report embeddings come from a synthetic device-resident embedding store "
                             "(builder/data/report_store.py); the loader hands over one report index per sample; "
                             "2: the same for the token ids of --berttype bert (TokenReportStore)")
    parser.add_argument("--val-iters", type=int, default=0,
                        help="N > 0: a validation pass of N synthetic batches at the end of every epoch (builder/trainer/validate.py, "
                             "DeviceEvaluator); 0: none")
    parser.add_argument("--val-batch-size", type=int, default=0, help="batch size of the validation pass (0: --batch-size)")
    args = parser.parse_args(argv)
    args.dir_root = os.getcwd()
    if int(args.synthetic) != 1:
        raise SystemExit("only --synthetic 1 is runnable here: the reference's data loaders need private MIMIC data "
                         "(SURVEY §2 row 9); builder/data/tie_dataset.py covers the vital-sign window construction")
    ddp = int(args.ddp) == 1
    val_iters, val_bs = int(args.val_iters), int(args.val_batch_size) or int(args.batch_size)
    if val_iters > 0 and ddp:
        raise SystemExit("--val-iters with --ddp 1: a sharded validation needs a gather of the evaluator state across the ranks, "
                         "which is not built (builder/trainer/validate.py refuses it)")
    rank, local, world = (int(os.environ.get(k, d)) for k, d in (("RANK", "0"), ("LOCAL_RANK", "0"), ("WORLD_SIZE", "1")))
    if not torch.cuda.is_available():
        raise SystemExit("training runs on an MI355X only (no CPU fallback)")
    if int(args.report_store) == 2 and args.berttype != "bert":
        raise SystemExit("--report-store 2 is the token-id store: it needs --berttype bert (--report-store 1 holds BioBERT embeddings)")
    if int(args.raw_images) in (2, 3):
        from .synthetic import jpeg_encode
        jpeg_encode(None)                              # fails here, by name, where PIL is not installed
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if ddp:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29541")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
    torch.manual_seed(int(args.seed_list[0]) if getattr(args, "seed_list", None) else 0)
    model, optimizer, criterion = build_training(args, device, ddp)
    n_it = int(args.iters_per_epoch)
    scheduler = CosineAnnealingWarmupRestarts(optimizer, first_cycle_steps=args.t_0 * n_it, cycle_mult=args.t_mult,
                                              max_lr=args.lr_init * math.sqrt(args.batch_size), min_lr=1e-6,
                                              warmup_steps=args.t_up * n_it, gamma=args.gamma)      # 2_train.py:118-124
    tie_store = None
    if int(args.tie_store) == 1:
        from .synthetic import make_tie_store
        tie_store = make_tie_store(4099).to(device)
        if rank == 0:
            print(f"event store: {tie_store.n_patients} patients, {tie_store.n_hours} hours, {tie_store.n_events} events, "
                  f"{tie_store.nbytes} bytes on {device}", flush=True)
    report_store = None
    if int(args.report_store) == 1:
        from .synthetic import make_report_store
        report_store = make_report_store(5003).to(device, getattr(model, "compute_dtype", torch.float32))
        if rank == 0:
            print(f"report store: {report_store.n_reports} reports, {report_store.n_tokens} tokens, {report_store.nbytes} bytes "
                  f"({report_store.dtype}) on {device}", flush=True)
    if int(args.report_store) == 2:
        from .synthetic import make_token_report_store
        report_store = make_token_report_store(5011, max_length=int(args.bert_token_max_length)).to(device)
        if rank == 0:
            print(f"token store: {report_store.n_reports} reports, {report_store.n_tokens} ids, {report_store.nbytes} bytes "
                  f"on {device}", flush=True)
    cxr_store = None
    if int(args.raw_images) == 3:
        from .synthetic import make_cxr_store
        cxr_store = make_cxr_store(6007 + rank).to(device)
        if rank == 0:
            print(f"image store: {cxr_store.n_images} images, {cxr_store.nbytes_streams} stream bytes, {cxr_store.nbytes_sync} "
                  f"sync-table bytes, {cxr_store.nbytes} bytes on {device}, built in {cxr_store.build_ms:.1f} ms", flush=True)
    logger, sweep = _Logger(), None
    if val_iters > 0:
        from .builder.trainer import validate
        from .builder.utils.device_evaluator import DeviceEvaluator
        logger = _Logger(DeviceEvaluator(args, device, val_iters * val_bs * int(args.output_dim)))
        if tie_store is not None:
            from .builder.data.tie_store import StoreWindowSweep
            sweep = StoreWindowSweep(tie_store, int(args.window_size))
    model.train()                                                                                    # 2_train.py:128
    iteration = 0
    for epoch in range(1, int(args.epochs) + 1):
        logger.loss, t0 = 0.0, time.perf_counter()
        for it, batch in enumerate(synthetic_loader(args, n_it, rank, epoch, tie_store, report_store, cxr_store), 1):
            x, static, y, in_len, img, img_time, txt, txt_len, txt_time, missing, _f, _y2 = batch
            iteration += 1
            model, iter_loss = get_trainer(args=args, iteration=iteration, x=x, static=static, input_lengths=in_len, y=y,
                                           output_lengths=None, model=model, logger=logger, device=device,
                                           scheduler=scheduler, optimizer=optimizer, criterion=criterion, x_txt=txt,
                                           x_img=img, txt_lengths=txt_len, imgtxt_time=(img_time, txt_time), scaler=None,
                                           missing=missing, flow_type="train", reports_tokens=None, reports_lengths=None,
                                           criterion_aux=(None, None))
            if not math.isfinite(iter_loss):
                raise SystemExit(f"non-finite loss at iteration {iteration}")
            logger.loss += iter_loss
            if rank == 0 and it % int(args.log_iter) == 0:
                print(f"epoch {epoch} iter {it}/{n_it} loss {logger.loss / it:.5f} lr {logger.lr:.3e}", flush=True)
        if rank == 0:
            dt = time.perf_counter() - t0
            print(f"epoch {epoch}: mean loss {logger.loss / n_it:.5f}, {world * args.batch_size * n_it / dt:.1f} samples/s "
                  f"(host-resident synthetic batches, H2D inside the step)", flush=True)
        if val_iters > 0:                                                                            # 2_train.py:213-290
            t0 = time.perf_counter()
            res = validate(args, model, synthetic_loader(args, val_iters, rank, 0, tie_store, report_store, cxr_store,
                                                         batch_size=val_bs, seed_base=VAL_SEED_BASE, sweep=sweep, train=False),
                           device, criterion, logger.evaluator)
            logger.val_loss = res["loss"]
            logger.add_validation_logs(iteration)
            if rank == 0:
                best = ", ".join(f"{v:.4f}" for v in logger.best_result_so_far) if logger.best_result_so_far else "-"
                print(f"epoch {epoch}: val loss {res['loss']:.5f} auroc {res['auroc']:.4f} ap {res['ap']:.4f} f1 {res['f1']:.4f} "
                      f"({res['n']} predictions, {res['n_pos']} positive, {time.perf_counter() - t0:.2f} s; best auc, apr, f1 "
                      f"[{best}] at iteration {logger.best_iter})", flush=True)
    gs = getattr(model, "_mtmp_graph_step", None)
    if rank == 0 and gs is not None:
        st = gs.stats()
        print(f"hipGraph: {st['captures']} captures, {st['replays']} replays, {st['eager_over_budget']} eager steps past the "
              f"capture budget", flush=True)
    ge = getattr(model, "_mtmp_graph_eval", None)
    if rank == 0 and ge is not None:
        st = ge.stats()
        print(f"hipGraph (validation): {st['captures']} captures, {st['replays']} replays, {st['eager_over_budget']} eager steps "
              f"past the capture budget", flush=True)
    if ddp:
        dist.destroy_process_group()
    return logger.loss / max(1, n_it)


if __name__ == "__main__":
    main(sys.argv[1:])
