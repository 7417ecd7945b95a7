"""Scheduling choices of the hot path, in ONE place (the A/B booleans were scattered over ops.py and trainer.py).

Each switch chooses the order in which independent launches are issued, or which of two launch sequences meant to be equivalent
runs.  The defaults below are what the tests and bench.py run, and the only settings they run: no test reads or sets one of these
attributes (HIP_HOURLY_EMBED, HIP_TRI_HEAD, HIP_ROW_HEAD and HIP_QIE excepted: their other setting is the reference's own torch chain, and a test runs both).  The other
settings are exercised only through ``tools/dbg/ab_patch.py`` (and the tools/dbg probes that flip one), so treat a non-default setting as unverified until such a run has compared it.  Each default is the faster setting as measured on
MI355X -- the measurement is named beside it and lives in DESIGN.md section 9 ("Built, measured, not kept").  They are module
attributes so that ab_patch.py can flip one and measure both settings on one machine in one session (machines differ by up to
5 %: an A/B across two sessions says nothing); product code reads them at call time, nothing else writes them.

A switch stays here only while its other setting is worth measuring again.  The four that forked the encoder layer engine (drop2's
backward folded into the dH launch, deferred and late gradient reductions, grouped against per-stream launches) and the two
stream issue orders nothing read are retired with the code their other setting selected: ops.layer_forward / ops.layer_backward
are the one engine, and DESIGN.md section 9 keeps their measurements and names the last commit that holds the code.

The two switches of the fusion stack and their one reader each, at call time: GROUP_MODE is read by ops.launch_groups() when a
layer's launch groups are made, FFN_ROWS_BEFORE_LAST by stack_plan.StackPlan.schedule() when a node's schedule is made.
"""

# How a layer's streams are cut into launches (bf16; the fp32 parity build launches per stream): "small" = the vital-sign stream
# alone on the caller's stream, image + text together on a side stream (8.57-8.93 ms); "all" = one launch over all three
# (9.2-9.36); "none" = one launch group per stream (8.78).
GROUP_MODE = "small"
# In the layer in front of a CLS-only last layer the image / text streams' FFN runs on the four rows the exchange reads (-0.05 ms).
FFN_ROWS_BEFORE_LAST = True
# builder/trainer: model.prefork() forks the frozen image encoder's stream at the head of the step, before zero_grad (-0.15 ms).
PREFORK_IMAGE_ENCODER = True
# mbt_encoder: the autograd node of the vital-sign stream's input kernel is created after the two short streams' ("long_last"), so
# that the backward issues it FIRST (autograd runs ready nodes latest-created first): the tail of the step is that stream's chain.
# "stream_order" = the order of round 4 (vital signs created first, issued last).  Measured in DESIGN section 7a.
INPUT_NODE_ORDER = "long_last"
# ops.StreamInputFn / ops.TieTimeEmbed backward: partial slabs + ONE mtmp_reduce_scatter launch that writes the parameters' slices of
# the flat gradient (the event and time embeddings' backward as one launch) instead of two reduction levels, a multi-tensor copy
# and the accumulation launches of the shared parameters per node.
FUSED_INPUT_TAIL = True
# tri_mbt_vsltcls (--berttype bert): the nn.Embedding(30000, 256) lookup and its gradient as ops.TokenEmbedFn (csrc/token_embed.hip:
# touched rows written into the flat gradient) instead of F.embedding + cast and embedding_dense_backward + AccumulateGrad (a dense
# [30000, 256] gradient built from zero and added: ~90 MB of traffic).  Forward bits are equal; profiles/token_embed.txt.
HIP_TOKEN_EMBED = True
# tri_mbt_vsltcls (--vslt-type carryforward): the hourly table's Linear(16, 256) -> LayerNorm -> ReLU as ops.HourlyEmbedFn (one
# launch forward, two backward, gradients into the flat buffer) instead of the torch chain (about ten launches each way plus four
# accumulations).  The one switch BOTH of whose settings the tests run (tests/test_carryforward_model_gpu.py): off is the torch
# chain the reference defines.  profiles/carryforward.txt.
HIP_HOURLY_EMBED = True
# tri_mbt_v1 / tri_mbt_vnoshavgtr (and tri_mbt_vnoshnoavgtr, whose masked loss needs a capturable chain either way): the three-row
# LayerNorm head and the candidate mean as ops.TriHeadFn + ops.CandidateMeanFn (csrc/head3.hip: three launches forward, four
# backward, one each way for the mean) instead of the torch chain stack -> LayerNorm -> cat -> Linear -> LayerNorm -> ReLU -> Linear
# -> four means -> gather plus ie_demo.  Like HIP_HOURLY_EMBED, BOTH settings are run by the tests (tests/test_noshnoavgtr_gpu.py):
# off is the torch chain the reference defines.  profiles/tri_head.txt.
HIP_TRI_HEAD = True
# tri_mbt_vflexible / 2 / 3, bitxt_ / biimg_mbt_vflexible1, tri_mbt_vmultivslt, tri_mbt_vmulti2: the LayerNorm head on two to four
# rows as ops.RowHeadFn (csrc/headr.hip: blocks of stream rows and a source table; ops.TriHeadFn for the three tri-modal flexible
# models) and the flexible models' softmax weighting over the present modalities as ops.FlexCombineFn (one launch each way)
# instead of the torch chain stack -> LayerNorm -> cat -> Linear -> LayerNorm -> ReLU -> Linear (-> masked_fill -> softmax -> four
# sums -> gather) plus ie_demo.  Like HIP_TRI_HEAD, BOTH settings are run by the tests (tests/test_flex_models_gpu.py): off is the
# torch chain the reference defines.  A model class opts out with ``hip_row_head = False``.  profiles/row_head.txt.
HIP_ROW_HEAD = True
# tri_mbt_vsltcls (--vslt-type QIE): the demographic rows of the three streams as ops.QieAddsFn (csrc/qie.hip: one launch forward,
# two backward), added inside the stream-input node (ops.StreamInputsQieFn), and the 256-wide BatchNorm head as ops.QieHeadFn
# (csrc/head.hip at width 256) -- with them the joint embedding node of TIE -- instead of the ie_demo torch chain, a [B,T,256] broadcast add with
# its summing backward, torch time embeddings and the torch head.  Like HIP_HOURLY_EMBED, BOTH settings are run by the tests
# (tests/test_qie_model_gpu.py): off is the torch chain the reference defines.  A model class opts in with ``hip_qie = True``.
# Step at B 64, TIE-len 1000, 6 layers, bf16, replayed: 8.95 ms (8.82-9.02) on against 9.51 ms (9.37-9.53) off, eight alternating
# windows in one process (tools/qie_bench.py; profiles/qie.txt).
HIP_QIE = True
# ops.layer_infer: the few-row FFN launches of a CLS-only last layer (B rows) and of the exchange-only layer in front of it (B * R
# rows) keep the training forward's two launches (mtmp_ln_gemm_signs + mtmp_gemm_nt) below this many rows instead of the fused
# mtmp_ffn_block: one workgroup of the fused kernel streams the whole megabyte of W1 and W2 for its 128 rows (42-44 us alone),
# the chain's kernels split the weights over many workgroups (34-35 us for both launches at 64 .. 3712 rows).  The fused launch
# reaches the chain only at 64 640 rows (115 against 117 us) and is slower at every smaller size measured (8768 rows: 47 against
# 39 us), so the bound is set above all of them.  tools/bench_kernels.py --only ffn_block; profiles/infer_forward.txt.
FFN_BLOCK_MIN_ROWS = 16384
