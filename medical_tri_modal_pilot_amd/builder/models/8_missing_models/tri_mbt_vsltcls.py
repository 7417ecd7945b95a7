"""TRI_MBT_VSLTCLS -- MI355X-native drop-in for the reference model of the same name
(builder/models/8_missing_models/tri_mbt_vsltcls.py:17-263).

Same constructor (``Model(args)``), same forward signature and return triple, same
parameter names/shapes (state_dicts load both ways).  The hot path runs on the HIP kernels
of libmtmp_hip.so: TIE/UMSE event embedding, Swin stem, LN-fused QKV/FFN projections,
key-length-masked flash attention and their backward passes.  Compute dtype is a build-only
flag (``args.compute_dtype``: "bf16" default, "fp32" = parity mode).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import contextlib

from medical_tri_modal_pilot_amd import ops, tuning
from medical_tri_modal_pilot_amd.builder.data.tie_dataset import PackedTie
from medical_tri_modal_pilot_amd.builder.models.src.swin_transformer import swin_t_m
from medical_tri_modal_pilot_amd.builder.models.src.transformer.mbt_encoder import TrimodalTransformerEncoder_MBT


def _compute_dtype(args) -> torch.dtype:
    name = str(getattr(args, "compute_dtype", "bf16")).lower()
    if name in ("bf16", "bfloat16"):
        return torch.bfloat16
    if name in ("fp32", "float32", "f32"):
        return torch.float32
    raise ValueError(f"--compute-dtype must be bf16 or fp32, got {name}")


def flat_layout(named, layer_stacks):
    """Order ``named`` parameters for optim.FlatParams: every encoder layer block in ops.PARAMS order -- (gamma,beta),
    (Wq,Wk,Wv), (bq,bk,bv), ... adjacent -- so that the backward kernels get contiguous gradient destinations
    (ops.GradSink); everything else keeps its place in front of / behind the blocks."""
    order = {}
    rank = [0, 1, 2, 5, 3, 6, 4, 7, 8, 9, 10, 11, 12, 13]     # param_list index -> position in the flat layout
    for li, layers in enumerate(layer_stacks):
        for m, layer in enumerate(layers):
            for k, q in enumerate(layer.param_list()):
                order[id(q)] = (li, m, rank[k])
    first = min((i for i, (_, q) in enumerate(named) if id(q) in order), default=len(named))
    head = [x for x in named[:first] if id(x[1]) not in order]
    body = sorted((x for x in named if id(x[1]) in order), key=lambda x: order[id(x[1])])
    tail = [x for x in named[first:] if id(x[1]) not in order]
    return head + body + tail


# The image / text input chains run on side streams on purpose (their backward tails overlap); autograd's warning
# about AccumulateGrad nodes living on another stream than their gradient's producer is expected then.
_quiet = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", None)
if _quiet is not None:
    _quiet(False)


class TRI_MBT_VSLTCLS(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.img_size = args.image_size
        self.patch_size = 16
        self.img_num_heads = 4
        self.output_dim = 1
        self.num_layers = args.transformer_num_layers
        self.num_heads = args.transformer_num_head
        self.model_dim = args.transformer_dim
        self.dropout = args.dropout
        self.idx_order = torch.arange(0, args.batch_size).type(torch.LongTensor)
        self.num_nodes = len(args.vitalsign_labtest)
        self.t_len = args.window_size
        self.device = args.device
        self.vslt_input_size = len(args.vitalsign_labtest)
        self.n_modality = len(args.input_types.split("_"))
        self.bottlenecks_n = 4
        self.compute_dtype = _compute_dtype(args)
        if self.model_dim != 256:
            raise ValueError("transformer_dim must be 256 (the reference hard-codes Linear(768,256) and "
                             "reshape(-1,147,256), tri_mbt_vsltcls.py:117,227-228)")
        self.activations = nn.ModuleDict([
            ["lrelu", nn.LeakyReLU()], ["prelu", nn.PReLU()], ["relu", nn.ReLU(inplace=True)], ["tanh", nn.Tanh()],
            ["sigmoid", nn.Sigmoid()], ["leaky_relu", nn.LeakyReLU(0.2)], ["elu", nn.ELU()]])

        # ---- encoders (reference :51-118)
        vslt_pe = self._make_embeddings(args)
        if args.berttype == "bert":
            self.txt_embedding = nn.Embedding(30000, self.model_dim)
        elif args.berttype == "biobert":
            self.txt_embedding = nn.Linear(768, self.model_dim)
        self.img_model_type = args.img_model_type
        self.img_pretrain = args.img_pretrain
        if self.img_model_type != "swin":
            raise NotImplementedError("only --img-model-type swin is on the MI355X hot path "
                                      "(vit / MONAI patch-embedding branches of tri_mbt_vsltcls.py:85-116 are out of scope)")
        # ImageNet / CXR-pretrained Swin weights come in through load_state_dict (no network, no /nfs path here).
        self.img_encoder = swin_t_m(compute_dtype=self.compute_dtype)
        self.img_encoder.eval()
        self.linear = nn.Linear(768, 256)
        self.flatten = nn.Flatten(1, 2)
        residual_bottlenecks = self.args.residual_bottlenecks == 1
        img_mask = self.args.multiimages == 1
        # ---- fusion (reference :129-145)
        self.fusion_transformer = TrimodalTransformerEncoder_MBT(
            batch_size=args.batch_size, n_modality=self.n_modality, bottlenecks_n=self.bottlenecks_n,
            fusion_startidx=args.mbt_fusion_startIdx, d_input=self.model_dim, resbottle=residual_bottlenecks,
            n_layers=self.num_layers, n_head=self.num_heads, d_model=self.model_dim, d_ff=self.model_dim * 4,
            dropout=self.dropout, vsltonly=self.args.mbt_only_vslt, pe_maxlen=2500,
            use_pe=[vslt_pe, False, True], mask=[True, img_mask, True], compute_dtype=self.compute_dtype)
        # forward() reads nothing of the encoder's result but the vital-sign stream's CLS row (reference :248), so the last
        # layer's image / text blocks are dead code on this path: the encoder neither runs them nor prepares their weights
        self.fusion_transformer.first_stream_output_only = True
        # ... which also means no pad row of the vital-sign stream is ever read: the stream may run packed (--pack-rows)
        self.fusion_transformer.pack_rows = bool(getattr(args, "pack_rows", 1))
        # ---- classifier (reference :147-158)
        classifier_dim = self.model_dim if self.args.vslt_type == "QIE" else self.model_dim * 2
        self.rmse_layer = nn.Linear(classifier_dim, 1, bias=True)
        self.layer_norms_after_concat = nn.LayerNorm(self.model_dim)
        self.fc_list = nn.Sequential(nn.Linear(classifier_dim, self.model_dim, bias=True),
                                     nn.BatchNorm1d(self.model_dim), self.activations["relu"],
                                     nn.Linear(self.model_dim, self.output_dim, bias=True))
        # number of images per sample: the reference hard-codes 3 (:161-162,226-231); generalised to K.
        self.n_images = int(getattr(args, "n_images", 3)) if self.args.multiimages == 1 else 1

    # --vslt-type QIE on HIP kernels (tuning.HIP_QIE: ops.QieAddsFn, ops.StreamInputsQieFn, ops.QieHeadFn).  Opt-in PER CLASS: forward()
    # asks the class's own dict, so a sibling that inherits forward() keeps the torch chain until it is pinned to goldens of its own.
    hip_qie = True
    head_fusable = True        # ie_demo = Linear -> LayerNorm -> ReLU: what ops.HeadFn fuses (a sibling may differ)
    head_min_train_batch = 2   # BatchNorm1d needs two rows in training mode (a sibling with a LayerNorm head: 1)
    # forward accepts a PackedTie in place of the padded x.  The trainer asks before it hands windows of the event store over
    # (trainer.py); a sibling that reads the padded tensor sets False, and a model class that does not define the flag at all is
    # given the padded form too.
    takes_packed_tie = True
    TRAINS_ENCODER_IN_REFERENCE = False      # this model and most siblings run the image encoder under no_grad (:205-209)

    def _make_embeddings(self, args) -> bool:
        """ie_vslt / ie_time / ie_feat / ie_demo in the reference's registration order (:51-76); returns vslt_pe."""
        def embed(n_in):
            return nn.Sequential(nn.Linear(n_in, self.model_dim), nn.LayerNorm(self.model_dim), nn.ReLU(inplace=True))

        if args.vslt_type == "carryforward":
            self.vslt_enc = embed(self.num_nodes)
            vslt_pe = True
        elif args.vslt_type in ("TIE", "QIE"):
            vslt_pe = False
            self.ie_vslt = embed(1)
        else:
            raise ValueError(args.vslt_type)
        self.ie_time = embed(1)
        self.ie_feat = nn.Embedding(20, self.model_dim)
        self.ie_demo = embed(2)
        return vslt_pe

    def _vslt_embedding(self, x, dt):
        """TIE / UMSE event embedding (:183-190): ReLU(LN(value w + b)) + ReLU(LN(time w + b)) + ie_feat[feature]."""
        tie_prm = (self.ie_vslt[0].weight, self.ie_vslt[0].bias, self.ie_vslt[1].weight, self.ie_vslt[1].bias,
                   self.ie_time[0].weight, self.ie_time[0].bias, self.ie_time[1].weight, self.ie_time[1].bias,
                   self.ie_feat.weight, dt)
        if isinstance(x, PackedTie):      # ragged batch of builder/data (events, cu_seqlens, t_pad), SURVEY 8 f-1
            return ops.TieEmbedPacked.apply(x.events, x.cu_seqlens, x.t_pad, *tie_prm)
        return ops.TieEmbed.apply(x, *tie_prm)                                                # [B,T,256]

    def _time_embeddings(self, img_time, txt_time, demo_embedding, dt):
        """(it [n_img,256], tt [B,256]): ie_time(t) + ie_feat[18 | 19] of every image / report time (:216-224)."""
        feat_tab = self.ie_feat.weight
        if (self.args.vslt_type == "QIE" and not getattr(self, "_qie_hip", False)) or not img_time.is_cuda:
            it = self.ie_time(img_time.unsqueeze(1)) + feat_tab[18]
            tt = self.ie_time(txt_time.unsqueeze(1)) + feat_tab[19]
            if self.args.vslt_type == "QIE":
                it = it + (demo_embedding if self.n_images == 1 else demo_embedding.repeat_interleave(self.n_images, 0))
                tt = tt + demo_embedding
            return it.to(dt), tt.to(dt)
        # both time embeddings of the batch in one HIP launch each way (ops.TimeEmbed)
        n_it = img_time.numel()
        ev = self._time_events(n_it, txt_time.numel(), img_time.device)
        ev[:, 0] = torch.cat([img_time, txt_time])
        emb = ops.TimeEmbed.apply(ev, self.ie_time[0].weight, self.ie_time[0].bias, self.ie_time[1].weight,
                                  self.ie_time[1].bias, feat_tab, dt)
        return emb[:n_it], emb[n_it:]

    joint_embeddings = True    # (switch for A/B runs and tests)
    defer_time_adds = True     # the time embeddings are added to their tokens inside the encoder's stream-input node

    def _joint_embeddings(self, x, img_time, txt_time, dt):
        """(vslt [B,T,256], it, tt) from ONE autograd node (ops.TieTimeEmbed) when the event embedding and the two time
        embeddings share ie_time / ie_feat and run as HIP kernels; None: the caller takes the two separate nodes."""
        if (not self.joint_embeddings or not (self.args.vslt_type == "TIE" or getattr(self, "_qie_hip", False))
                or isinstance(x, PackedTie) or not img_time.is_cuda or not x.is_cuda):
            return None
        n_it = img_time.numel()
        ev = self._time_events(n_it, txt_time.numel(), img_time.device)
        ev[:, 0] = torch.cat([img_time, txt_time])
        return ops.TieTimeEmbed.apply(x, ev, n_it, self.ie_vslt[0].weight, self.ie_vslt[0].bias, self.ie_vslt[1].weight,
                                      self.ie_vslt[1].bias, self.ie_time[0].weight, self.ie_time[0].bias, self.ie_time[1].weight,
                                      self.ie_time[1].bias, self.ie_feat.weight, dt)

    # NOTE: like the reference, model.train() (2_train.py:128) puts the Swin encoder back into train mode
    # although the constructor called .eval() (:104), so its row-mode StochasticDepth is active while
    # training.  Parity tests call model.img_encoder.eval() explicitly, as the golden generator did.

    def hot_parameters(self):
        """Parameters that receive a gradient on this path (what AdamW updates and DDP all-reduces):
        excludes the frozen Swin, the last layer's image/text blocks when --mbt-only-vslt 1, and the
        heads the forward never touches (SURVEY.md §2b parameter census)."""
        L = self.num_layers
        skip = ["img_encoder.", "fusion_transformer.layer_norms_after_concat.", "activations."]
        if "rmse" not in self.args.auxiliary_loss_type:
            skip.append("rmse_layer.")
        # the last layer's image / text blocks never reach the loss: skipped outright with --mbt-only-vslt 1
        # (mbt_encoder.py:757-763), computed but unread otherwise (only outputs[0][:, 0, :] feeds the head,
        # tri_mbt_vsltcls.py:248) -- their gradient is None in the reference, so AdamW leaves them alone
        skip += [f"fusion_transformer.layer_stacks.{L - 1}.1.", f"fusion_transformer.layer_stacks.{L - 1}.2."]
        named = [(n, p) for n, p in self.named_parameters() if not n.startswith(tuple(skip))]
        return flat_layout(named, self.fusion_transformer.layer_stacks)

    def backward_stage_params(self, lo: int, hi: int, head: bool):
        """Trained parameters used by the fusion layers [lo, hi) (and the classifier head): what a staged backward
        (builder/trainer: one hipGraph per group of layers) lets autograd accumulate into while it stops at the
        stream buffers in front of layer ``lo``."""
        pre = tuple(f"fusion_transformer.layer_stacks.{l}." for l in range(lo, hi))
        if head:
            pre += ("ie_demo.", "layer_norms_after_concat.", "fc_list.", "rmse_layer.")
        return [p for n, p in self.named_parameters() if p.requires_grad and n.startswith(pre)]

    def _time_events(self, n_img: int, n_txt: int, device) -> torch.Tensor:
        """[n_img + n_txt, 3] event rows (time, 0, modality id 18 | 19) for ops.TimeEmbed; the id column is constant."""
        key = (n_img, n_txt, str(device))
        if getattr(self, "_tev_key", None) != key:
            ev = torch.zeros(n_img + n_txt, 3, device=device)
            ev[:n_img, 2], ev[n_img:, 2] = 18.0, 19.0
            self._tev, self._tev_key = ev, key
        return self._tev.clone()

    def prefork(self, img):
        """Optional, for the trainer: called before anything else of a training step is issued on the current stream (the
        inputs are in place).  The frozen image encoder is the head of the step's critical path and needs nothing but the
        images, so its stream is forked HERE -- not behind zero_grad, the dropout-seed update and the text projection, ~75 us
        of small launches in front of the first encoder kernel -- and the StochasticDepth draws (four small launches) run on
        the caller's stream beside the patch embedding instead of in front of it.  forward() then skips its own fork."""
        self._preforked = False
        # the same predicate as forward(): the fork only exists when the input chains run on the encoder's side streams
        side = (None if (not img.is_cuda or not getattr(self, "side_input_chains", True))
                else self.fusion_transformer._side_streams(img.device))
        if side is None or self.args.img_model_type != "swin":
            return
        cur = torch.cuda.current_stream()
        if getattr(self, "_swin_stream", None) is None or self._swin_stream.device != img.device:
            self._swin_stream = torch.cuda.Stream(device=img.device)
        self._swin_stream.wait_stream(cur)
        n = img.numel() // (img.shape[-2] * img.shape[-1])
        self.img_encoder.predraw(n, img.device)
        self._preforked = True

    def forward(self, x, h, m, d, x_m, age, gen, input_lengths, txts, txt_lengths, img, missing, f_indices, img_time,
                txt_time, flow_type, reports_tokens, reports_lengths):
        dt = self.compute_dtype
        ops.mark("fwd.s")
        preforked, self._preforked = getattr(self, "_preforked", False), False     # (cleared whatever branch runs below)
        if isinstance(x, PackedTie):
            if self.args.vslt_type == "carryforward":
                raise ValueError("a packed TIE batch needs --vslt-type TIE or QIE")
            B = x.cu_seqlens.numel() - 1
        else:
            B = x.size(0)
            x = x.float()
        age, gen = age.float(), gen.float()
        # head + ie_demo as six HIP launches (ops.HeadFn) when the demographic embedding feeds nothing but the head
        fused_head = (self.head_fusable and age.is_cuda and B <= ops.HEAD_MAX_B and self.args.vslt_type != "QIE"
                      and "rmse" not in self.args.auxiliary_loss_type and (B >= self.head_min_train_batch or not self.training))
        if (not fused_head and self.head_fusable and age.is_cuda and self.training and not getattr(self, "_warned_torch_head", False)
                and self.args.vslt_type != "QIE" and "rmse" not in self.args.auxiliary_loss_type):
            import warnings
            self._warned_torch_head = True
            warnings.warn(f"{type(self).__name__}: batch of {B} is outside the fused head kernels' range ({self.head_min_train_batch} <= B <= {ops.HEAD_MAX_B} in "
                          "training): the classifier head runs as torch ops (same results, ~60 more small launches per step)")
        # --vslt-type QIE on its HIP nodes (class attribute hip_qie above; tuning.HIP_QIE): one image per sample, a batch the head
        # kernels take, the fused stream-input node in the encoder.  Anything else is the torch chain below, as before.
        enc_ = self.fusion_transformer
        qie_hip = self._qie_hip = bool(
            self.args.vslt_type == "QIE" and tuning.HIP_QIE and vars(type(self)).get("hip_qie", False) and age.is_cuda
            and self.n_images == 1 and B <= ops.HEAD_MAX_B and (B > 1 or not self.training)
            and "rmse" not in self.args.auxiliary_loss_type and tuning.FUSED_INPUT_TAIL and self.defer_time_adds
            and min(max(enc_.fusion_idx, 0), enc_.n_layers) == 0 and enc_.n_layers > 0 and getattr(enc_, "n_modality", 0) == 3
            and (isinstance(x, PackedTie) or x.is_cuda) and img_time.is_cuda and txt_time.is_cuda)
        demo_embedding = None
        if not fused_head and not qie_hip:
            demographic = torch.stack([age, gen], dim=1)
            demo_embedding = self.ie_demo(demographic)                                        # [B,256] fp32
        # The image and text input chains (projection, time embedding add, and -- inside the encoder -- the stream
        # input kernel) are issued on the encoder's two side HIP streams: autograd runs a node's backward on the
        # stream of its forward, so the three modalities' input-side backward tails (all small, latency-bound
        # launches at the very end of the step) run side by side instead of one after the other.
        side = (None if (not txts.is_cuda or not getattr(self, "side_input_chains", True))
                else self.fusion_transformer._side_streams(txts.device))
        cur = torch.cuda.current_stream() if side is not None else None
        on_side = (lambda k: torch.cuda.stream(side[k])) if side is not None else (lambda k: contextlib.nullcontext())
        if side is not None:
            for s_ in side:
                s_.wait_stream(cur)
        # ---- text stream: projection of the pre-computed BioBERT token embeddings (:200)
        with on_side(1):
            if self.args.berttype == "biobert":
                te = self.txt_embedding
                txt_embedding = ops.DataLinearFn.apply(txts, te.weight, te.bias, dt)
            elif tuning.HIP_TOKEN_EMBED and txts.is_cuda:
                # token ids (--berttype bert, :202): the trained nn.Embedding(30000, 256) as a HIP gather whose backward
                # writes the touched rows of the table's gradient (ops.TokenEmbedFn)
                txt_embedding = ops.TokenEmbedFn.apply(txts, self.txt_embedding.weight, dt)
            else:
                txt_embedding = self.txt_embedding(txts).to(dt)
        # ---- image stream: frozen Swin-T -> [B*K,7,7,768] -> flatten -> Linear(768,256) (:205-211)
        if self.args.multiimages == 1:
            img = img.reshape(-1, 1, img.shape[-2], img.shape[-1])
        # The frozen encoder itself runs on the image side stream: nothing of the vital-sign stream depends on it before
        # the first bottleneck exchange, so the main stream goes on (TIE embedding, stream input, the vital-sign
        # stream's first layer) beside the encoder's small-M stages, which cannot fill the chip on their own.
        # Samples without an image (missing_num 2 / 3: the bottleneck exchange gives their image stream weight 0, and this
        # model reads nothing else of it) are not encoded: the present images take the first slots of the encoder's batch
        # (ops.image_slots), the others come back as zero features.  The reference encodes a zero image for them.
        # With --multiimages 1 the image stream's key length is 4 + 1 + 49 * (images whose time is not the pad value 10), :226-231:
        # the tokens of image j >= that count are masked as keys and read by nothing -- those images are not encoded either
        # (by POSITION, as the reference masks them; an image in front of the count is encoded whatever its time says).
        # (image sides that are multiples of 32, 224 and 512 among them: every stage's map halves exactly, so that hw0 >> 2s is
        #  the slot table's row count per image at stage s; other sizes -- 200 pixels: 50 -> 25 -> 13 -> 7 -- encode every image)
        skip = (bool(getattr(self.args, "skip_missing_images", 1)) and img.is_cuda
                and self.args.img_model_type == "swin" and torch.is_tensor(missing) and missing.dim() == 1
                and img.shape[-2] % 32 == 0 and img.shape[-1] % 32 == 0)

        def encode(**kw):
            slots = None
            hw0 = (img.shape[-2] // 4) * (img.shape[-1] // 4)
            if skip and self.args.multiimages == 1:
                K = self.n_images
                n_keep = torch.count_nonzero(img_time.reshape(-1, K).to(img.device) - 10, dim=1)            # [B]
                absent = (torch.arange(K, device=img.device).unsqueeze(0) >= n_keep.unsqueeze(1)).reshape(-1)
                slots = ops.image_slots(absent.to(torch.int64), 1, hw0)
            elif skip:
                # missing_num 0: all three modalities, 1: vital signs + image (builder/trainer missing_to_num)
                slots = ops.image_slots(missing.to(img.device), 2, hw0)
            return self.img_encoder(img, slots=slots, **kw)
        trained = self.TRAINS_ENCODER_IN_REFERENCE and self.img_encoder.trains()
        if trained:
            # sibling models whose reference back-propagates into the encoder (tri_mbt_v2.py:208-211): the autograd path of the
            # encoder (SwinTransformer.forward_train), every image encoded, the feature projection passing its input gradient on
            with on_side(0):
                feat = self.flatten(self.img_encoder(img))
                img_embedding = ops.LinearFn.apply(feat, self.linear.weight, self.linear.bias, dt)
        elif side is not None:
            # stages 1-2 on a third stream, stages 3-4 as two half batches on the two side streams (result valid on side[0])
            if not preforked:                             # (prefork() joined the encoder's stream at the head of the step)
                if getattr(self, "_swin_stream", None) is None or self._swin_stream.device != img.device:
                    self._swin_stream = torch.cuda.Stream(device=img.device)
                self._swin_stream.wait_stream(cur)
            with torch.cuda.stream(self._swin_stream), torch.no_grad():
                ops.mark("swin.s")
                feat = encode(tail_streams=(side[0], side[1]))
            side[0].wait_stream(self._swin_stream)        # (already implied when the encoder split its tail)
            with on_side(0):
                feat = self.flatten(feat)
                ops.mark("swin.e")
        else:
            with torch.no_grad():
                feat = encode()
            feat = self.flatten(feat)
        if not trained:
            with on_side(0):
                img_embedding = ops.DataLinearFn.apply(feat, self.linear.weight, self.linear.bias, dt)
        # ---- vital-sign / lab stream
        img_time = img_time.reshape(-1).float()
        txt_time = txt_time.float()
        it = tt = None
        if self.args.vslt_type == "carryforward":
            if tuning.HIP_HOURLY_EMBED and x.is_cuda:
                # the hourly table's Linear -> LayerNorm -> ReLU (:51-57,179-181) as one HIP launch each way (ops.HourlyEmbedFn)
                enc = self.vslt_enc
                vslt_embedding = ops.HourlyEmbedFn.apply(x, enc[0].weight, enc[0].bias, enc[1].weight, enc[1].bias, dt)
            else:
                vslt_embedding = self.vslt_enc(x).to(dt)
        else:
            joint = self._joint_embeddings(x, img_time, txt_time, dt) if self.args.imgtxt_time == 1 else None
            if joint is not None:
                vslt_embedding, it, tt = joint
            else:
                vslt_embedding = self._vslt_embedding(x, dt)
            if self.args.vslt_type == "QIE" and not qie_hip:
                vslt_embedding = vslt_embedding + demo_embedding.unsqueeze(1).to(dt)
        if self.args.imgtxt_time == 1:                                                        # (:216-224)
            if it is None:
                it, tt = self._time_embeddings(img_time, txt_time, demo_embedding, dt)
            if side is not None:
                for s_ in side:
                    s_.wait_stream(cur)              # the time embeddings were made on the main stream
            # added to every token of its image / report inside the encoder's stream-input node (mbt_encoder ``time_adds``), whose
            # backward then hands the embedding node its gradient without two more autograd nodes on the step's tail
            defer_add = (self.defer_time_adds and it.is_cuda and it.dim() == 2 and tt.dim() == 2
                         and getattr(self.fusion_transformer, "n_modality", 0) == 3)
            if not defer_add:
                with on_side(0):
                    img_embedding = img_embedding + it.unsqueeze(1)
                with on_side(1):
                    txt_embedding = txt_embedding + tt.unsqueeze(1)
        if self.args.multiimages == 1:                                                        # (:226-232)
            n_tok = img_embedding.shape[1]
            img_embedding = img_embedding.reshape(B, self.n_images * n_tok, self.model_dim)
            img_len = torch.count_nonzero(img_time.reshape(B, self.n_images) - 10, dim=1) * n_tok
        else:
            img_len = img_embedding.size(1)
        self.fusion_transformer.inputs_on_side_streams = side is not None
        self.fusion_transformer.time_adds = (it, tt) if (self.args.imgtxt_time == 1 and defer_add) else None
        if qie_hip:
            # demo, it + demo, tt + demo as ONE launch (ops.QieAddsFn), added to every token inside the stream-input node, whose backward
            # leaves its input gradients in ``handoff`` for that node's two backward launches (:191-198, 216-221)
            if self.args.imgtxt_time == 1 and not defer_add:
                raise RuntimeError("QIE on the HIP path adds the time embeddings inside the stream-input node")
            dm, handoff = self.ie_demo, {}
            adds = ops.QieAddsFn.apply(age, gen, it if self.args.imgtxt_time == 1 else None, tt if self.args.imgtxt_time == 1 else None,
                                       dt, handoff, dm[0].weight, dm[0].bias, dm[1].weight, dm[1].bias)
            if side is not None:
                for s_ in side:
                    s_.wait_stream(cur)              # the add rows were made on the main stream
            self.fusion_transformer.time_adds = None
            self.fusion_transformer.qie_adds = (*adds, handoff)
        ops.mark("inputs.e")
        outputs, _ = self.fusion_transformer(
            enc_outputs=[vslt_embedding, img_embedding, txt_embedding],
            fixed_lengths=[vslt_embedding.size(1), img_embedding.size(1), txt_embedding.size(1)],
            varying_lengths=[input_lengths, img_len, txt_lengths + 2], fusion_idx=None, missing=missing)
        if side is not None and not trained:
            cur.wait_stream(self._swin_stream)            # joins the encoder's stream to the caller's (its work ended long ago)
        return self._head(outputs, demo_embedding, age, gen, missing, fused_head)

    def _head(self, outputs, demo_embedding, age, gen, missing, fused_head):
        """The classifier on the encoder's result (:248-255), fp32 -- a hook: sibling models read other rows."""
        cls = self.fusion_transformer.last_cls             # outputs[0][:, 0, :] as a dedicated autograd output
        cls = outputs[0][:, 0, :] if cls is None else cls
        ops.mark("stack.e")
        if fused_head:
            # (the kernels read the CLS vectors in the fusion stack's type and count the batch themselves)
            bn, ln, dm = self.fc_list[1], self.layer_norms_after_concat, self.ie_demo
            nbt = bn.num_batches_tracked if (bn.training and bn.track_running_stats) else None
            if nbt is not None and not nbt.is_cuda:
                nbt.add_(1)
                nbt = None
            use_batch = bn.training or not bn.track_running_stats
            output1 = ops.HeadFn.apply(cls, age, gen, use_batch, 0.1 if bn.momentum is None else bn.momentum, bn.eps,
                                       bn.running_mean, bn.running_var, nbt, dm[0].weight, dm[0].bias, dm[1].weight, dm[1].bias,
                                       ln.weight, ln.bias, self.fc_list[0].weight, self.fc_list[0].bias, bn.weight, bn.bias,
                                       self.fc_list[3].weight, self.fc_list[3].bias)
            return output1, None, None
        if getattr(self, "_qie_hip", False) and vars(type(self)).get("hip_qie", False):
            # the 256-wide BatchNorm head (ops.QieHeadFn): HeadFn's forms without the ie_demo half
            bn, ln = self.fc_list[1], self.layer_norms_after_concat
            nbt = bn.num_batches_tracked if (bn.training and bn.track_running_stats) else None
            if nbt is not None and not nbt.is_cuda:
                nbt.add_(1)
                nbt = None
            use_batch = bn.training or not bn.track_running_stats
            output1 = ops.QieHeadFn.apply(cls, use_batch, 0.1 if bn.momentum is None else bn.momentum, bn.eps, bn.running_mean,
                                          bn.running_var, nbt, ln.weight, ln.bias, self.fc_list[0].weight, self.fc_list[0].bias,
                                          bn.weight, bn.bias, self.fc_list[3].weight, self.fc_list[3].bias)
            return output1, None, None
        cls = cls.float()
        class_input = self.layer_norms_after_concat(cls)
        if self.args.vslt_type != "QIE":
            class_input = torch.cat([class_input, demo_embedding], dim=1)
        output2 = self.rmse_layer(class_input).squeeze() if "rmse" in self.args.auxiliary_loss_type else None
        output1 = self.fc_list(class_input)
        return output1, output2, None
