"""TRI_MBT_VMULTI2 -- MI355X-native drop-in for the reference's second multi-token tri-modal MBT model
(builder/models/8_missing_models/tri_mbt_vmulti2.py:10-179).

TRI_MBT_VMULTIVSLT with three differences:
  * the Swin-T image encoder is TRAINED (the reference calls it outside no_grad, :145): its 171 parameter tensors are
    ``hot_parameters()`` and every image is encoded on the encoder's autograd path;
  * all three streams are masked (``mask=[True] * 3``, :114) and all three outputs are read, so no block of the last layer is dead;
  * the heads' inputs (:161-165): head 0 the mean of the three streams' row 0, head 1 the mean of the vital-sign stream's row 1 and
    the image stream's row 1, head 2 the mean of the vital-sign stream's row 2 and the text stream's row 1, head 3 the vital-sign
    stream's row 3.  Rows 1 of the image and text streams are TOKEN rows there (those streams carry no CLS rows); kept as it is.
``rmse_layer`` exists (:120) and is used only with an rmse auxiliary loss, which this path refuses like the reference's trainer
does for these models.  The heads are ops.RowHeadFn on three blocks under tuning.HIP_ROW_HEAD (the source means are taken inside
its first kernel), the torch chain otherwise.
"""
import torch
import torch.nn as nn

from .tri_mbt_vmultivslt import TRI_MBT_VMULTIVSLT
from .tri_mbt_vsltcls import flat_layout


class TRI_MBT_VMULTI2(TRI_MBT_VMULTIVSLT):
    TRAINS_ENCODER_IN_REFERENCE = True
    MASKS = [True, True, True]
    FIRST_STREAM_ONLY = False
    # blocks v[:, :4], i[:, :2], t[:, :2]; head 0 = mean(v0, i0, t0), head 1 = mean(v1, i1), head 2 = mean(v2, t1), head 3 = v3
    HEAD_TABLE = (((0, 0), (1, 0), (2, 0)), ((0, 1), (1, 1)), ((0, 2), (2, 1)), ((0, 3),))

    def _head_blocks(self, outputs):
        v, i, t = outputs
        return [v[:, :4, :], i[:, :2, :], t[:, :2, :]]

    def _make_heads(self):
        self.rmse_layer = nn.Linear(self.model_dim * 2, 1, bias=True)
        super()._make_heads()

    def hot_parameters(self):
        skip = ["img_encoder.head.", "fusion_transformer.layer_norms_after_concat.", "activations.", "rmse_layer."]
        named = [(n, p) for n, p in self.named_parameters() if not n.startswith(tuple(skip))]
        return flat_layout(named, self.fusion_transformer.layer_stacks)

    def _head_rows(self, outputs):
        v, i, t = outputs
        tri = torch.stack([v[:, 0, :], i[:, 0, :], t[:, 0, :]]).float().mean(0)
        vi = torch.stack([v[:, 1, :], i[:, 1, :]]).float().mean(0)
        vt = torch.stack([v[:, 2, :], t[:, 1, :]]).float().mean(0)
        return torch.stack([tri, vi, vt, v[:, 3, :].float()])
