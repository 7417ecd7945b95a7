"""Ragged collate / data path of the TIE (continuous-time vital-sign / lab event) stream -- SURVEY 8 f-1.

``tie_window`` restates the TIE branch of ``Multiple_Outbreaks_Training_Dataset.__getitem__``
(/root/reference builder/data/dataset_new.py:1969-2030); ``PackedTieBatch`` replaces the zero-padded
``[B, TIE_len, 3]`` batch tensor by ``(events[sum T, 3], cu_seqlens[B + 1])`` on pinned host memory."""
import torch


def resolve_device(device) -> torch.device:
    """``device`` as a ``torch.device`` that names ONE device: "cuda" becomes ``cuda:<current>``, what a tensor put there reports as
    its own, so that a store's ``device`` compares equal to its tensors'.  Everything else is returned as given.  (Defined ahead of
    the imports below: the store modules import it from here.)"""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


from .tie_dataset import (PackedTie, PackedTieBatch, SampleTieDataset, collate_packed, tie_window)  # noqa: E402,F401
from .tie_store import (HourlyWindowBatch, StoreWindowDataset, StoreWindowSweep, TieEventStore, TieWindowBatch,  # noqa: F401
                        collate_hourly_windows, collate_windows, keep_mask)
from .report_store import ReportBatch, ReportStore, TokenReportBatch, TokenReportStore, report_wanted  # noqa: F401
from .cxr_store import CxrImage, CxrStore, CxrStoreBatch, image_wanted  # noqa: F401
from .jpeg import JpegInfo, JpegPlan, parse_jpeg  # noqa: F401
from .cxr_transform import (CxrRandomTransform, CxrTransform, RawCxrBatch, collate_raw_cxr, draw_affine, draw_randaug,  # noqa: F401
                            draw_resized_crop, transform_from_args)
