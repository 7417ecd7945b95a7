"""TRI_MBT_VNOSHNOAVGTR -- MI355X-native drop-in for the reference's tri-modal MBT model that hands out the three modality heads'
logits UN-AVERAGED (builder/models/8_missing_models/tri_mbt_vnoshnoavgtr.py:17-283).

TRI_MBT_VNOSHAVGTR in everything but the last lines of the forward: same constructor, same parameter names (state_dicts load both
ways with the reference class), the Swin-T image encoder trained, one head per modality.  The forward returns
``torch.stack(outputs)`` = [3, B, 1] (:259-281): no candidate mean in the model.  The reference's ``missing_trainer`` consumes that
shape in a branch keyed on ``"mbt_vnoshnoavgtr" in args.model``:

  * train (builder/trainer/trainer.py:169-174): the target repeated over the three rows, BCE over the logits of the modalities that
    are present (``output[original_missing == 0]``) -- every head gets its own supervised signal;
  * test (:223-230): the four candidate means built in the trainer and gathered by ``missing_num``.

Here the trainer takes ops.bce_masked_mean / ops.candidate_mean for the two (builder/trainer/trainer.py), both of which read the
present modalities off ``missing_num``: S(0) = {vslt, img, txt}, S(1) = {vslt, img}, S(2) = {vslt, txt}, S(3) = {vslt}.  That is the
reference's mask ``missing.T == 0`` only when ``missing_num`` is computed from all three flags and nothing is folded, so the
constructor asks for ``--input-types vslt_img_txt --fullmodal-definition txt1_img1``.
"""
from medical_tri_modal_pilot_amd import ops

from .tri_mbt_vnoshavgtr import TRI_MBT_VNOSHAVGTR


class TRI_MBT_VNOSHNOAVGTR(TRI_MBT_VNOSHAVGTR):
    def __init__(self, args):
        if args.input_types != "vslt_img_txt":
            raise NotImplementedError(f"TRI_MBT_VNOSHNOAVGTR needs --input-types vslt_img_txt (got {args.input_types}): its training loss "
                                      "masks the three heads' logits by the modalities that are present, and the trainer folds the "
                                      "pattern ids of a two-modality run (trainer.py:99-105)")
        if getattr(args, "fullmodal_definition", "txt1_img1") != "txt1_img1":
            raise NotImplementedError(f"TRI_MBT_VNOSHNOAVGTR needs --fullmodal-definition txt1_img1 (got {args.fullmodal_definition}): "
                                      "only then do the pattern ids say which of the three modalities are present "
                                      "(trainer.py:53-77,169-174)")
        super().__init__(args)

    @property
    def head_fusable(self):
        """always the head kernels where they apply: the masked loss behind them is what makes the step capturable"""
        return True

    def _head(self, outputs, demo_embedding, age, gen, missing, fused_head):
        if fused_head:
            return self._tri_logits(outputs, age, gen, self.fc_lists).unsqueeze(-1), None, None
        o, output2 = self._torch_logits(outputs, demo_embedding)
        return o, output2, None
