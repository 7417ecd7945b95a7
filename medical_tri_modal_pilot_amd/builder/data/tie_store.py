"""The TIE event windows of a whole data set, built on the device from a device-resident event store.

``tie_window`` (tie_dataset.py) builds one window per call on the host: it normalises the patient's hourly table, concatenates the
hourly event arrays, shifts and truncates.  After trimming, a window is at most 18 carried-forward "initial" rows followed by a
CONTIGUOUS run of the patient's events with the times shifted by one scalar -- so the data set is stored once (``TieEventStore``,
CSR over patients -> hours -> events), a window is three int32 ``(patient, selected_key, rand_length)``, the host resolves
the control flow of a batch of them on the hour-level arrays alone (``TieEventStore.plan`` -> ``TieWindowBatch``, vectorised, no
event is touched) and one kernel launch (``ops.tie_windows`` -> csrc/tie_store.hip) writes what ``mtmp_tie_embed_packed_fwd`` reads.

What is stored, and why the result has the bits of ``tie_window``:
  * ``norm`` [H, 18] float32: ``(data - mins) / (maxs - mins)`` evaluated in float64 by the numpy expression of ``tie_window`` and
    rounded to float32 once -- the rounding ``tie_window`` applies to the initial rows' values;
  * ``delta`` [H, 18] float64 and event times float64: the reference subtracts the prediction hour in float64 and rounds after;
  * event values float32 (the one rounding of ``ev.astype(np.float32)``), feature indices uint8 (checked at build time to be the
    integers 0..255 with a clear sign bit, whose float32 form is exact);
  * ``present`` [H]: a ``None`` hour is not an empty hour, the trimming depends on it;
  * ``hour_min`` [H] float64: the earliest event time of the hour (+inf without events), for the ``realtime != 1`` shift.

The same store serves ``--vslt-type carryforward``: the loader's hourly table of a window (dataset_new.py:2006-2011) is a
contiguous run of rows of ``norm`` in the kept columns, padded with zero rows -- ``TieEventStore.plan_hourly`` ->
``HourlyWindowBatch`` (the same triples, the same refusals, the ``None``-hour trimming shared with ``plan`` for the text time) and
``ops.hourly_windows`` (one launch, csrc/tie_store.hip).
"""
import glob
import os
import pickle
import random
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import resolve_device

N_FEAT = 18
DESC_WORDS = 8      # int64 words per sample of the kernel's descriptor (include/mtmp.h, mtmp_tie_window_gather)
(DESC_FIRST_EVENT, DESC_N_EVENTS, DESC_INIT_HOUR, DESC_FIRST_HOUR, DESC_N_HOURS, DESC_MASK, DESC_T0, DESC_KEY) = range(DESC_WORDS)


class TieWindowBatch:
    """The host plan of a batch of windows: everything but the events.  ``ops.tie_windows`` turns it into a ``PackedTie`` (or the
    padded tensor) on the device; lengths and ``max_len`` are here without a device sync."""

    def __init__(self, store, windows, first_event, n_events, init_mask, init_hour, first_hour, n_hours, selected_key, t0, first,
                 input_lengths, cu_seqlens, txt_time, static, tie_len, realtime):
        self.store, self.windows = store, windows
        self.first_event, self.n_events, self.init_mask = first_event, n_events, init_mask
        self.init_hour, self.first_hour, self.n_hours = init_hour, first_hour, n_hours
        self.selected_key, self.t0, self.first = selected_key, t0, first
        self.input_lengths, self.cu_seqlens, self.txt_time, self.static = input_lengths, cu_seqlens, txt_time, static
        self.tie_len, self.realtime = int(tie_len), int(realtime)

    @property
    def batch_size(self) -> int:
        return int(self.input_lengths.numel())

    @property
    def max_len(self) -> int:
        return int(self.input_lengths.max())

    @property
    def total_rows(self) -> int:
        return int(self.cu_seqlens[-1])

    def descriptor(self) -> torch.Tensor:
        """int64 [B, DESC_WORDS]: the per-sample words of mtmp_tie_window_gather."""
        d = np.stack([self.first_event, self.n_events, self.init_hour, self.first_hour, self.n_hours,
                      self.init_mask.astype(np.int64), self.t0, self.selected_key], axis=1).astype(np.int64)
        return torch.from_numpy(np.ascontiguousarray(d))


DEFAULT_DROPPED = (6, 17)   # the two columns of the 18 whose names the default --vitalsign-labtest omits


def keep_mask(feature_order: Sequence[str], wanted_names: Sequence[str]) -> np.ndarray:
    """bool [len(feature_order)]: which columns of a pickle's table ``--vitalsign-labtest`` keeps (the reference's
    ``args.vslt_mask``), from the pickle's own ``feature_order`` field."""
    order = [str(n) for n in feature_order]
    wanted = [str(n) for n in wanted_names]
    unknown = [n for n in wanted if n not in order]
    if unknown:
        raise ValueError(f"keep_mask: {unknown} not in feature_order {order}")
    return np.asarray([n in wanted for n in order], bool)


def _keep_bits(keep) -> int:
    """``keep`` (None | 18 booleans | column indices) -> the kernel's bit mask over the 18 columns."""
    if keep is None:
        cols = [f for f in range(N_FEAT) if f not in DEFAULT_DROPPED]
    else:
        k = np.asarray(keep)
        if k.dtype == bool:
            if k.shape != (N_FEAT,):
                raise ValueError(f"plan_hourly: a boolean keep has {N_FEAT} entries, got {k.shape}")
            cols = np.flatnonzero(k).tolist()
        else:
            if k.ndim != 1 or k.dtype.kind not in "iu":
                raise ValueError(f"plan_hourly: keep is {N_FEAT} booleans or a list of column indices, got {k.dtype} {k.shape}")
            cols = [int(c) for c in k]
            if any(c < 0 or c >= N_FEAT for c in cols) or len(set(cols)) != len(cols) or cols != sorted(cols):
                raise ValueError(f"plan_hourly: keep indices must be distinct, ascending and inside 0..{N_FEAT - 1}, got {cols}")
    if not cols:
        raise ValueError("plan_hourly: keep selects no column")
    return sum(1 << int(c) for c in cols)


class HourlyWindowBatch:
    """The host plan of a batch of hourly carry-forward windows (``--vslt-type carryforward``): sample b is rows
    ``first_row .. first_row + n_rows - 1`` of ``store.norm``, columns ``keep_bits``, then zero rows up to ``window_size``.
    ``ops.hourly_windows`` writes the float32 [B, window_size, n_feat] table on the device; the lengths are here."""

    def __init__(self, store, windows, first_row, n_rows, input_lengths, txt_time, static, window_size, keep_bits, realtime):
        self.store, self.windows, self.first_row, self.n_rows = store, windows, first_row, n_rows
        self.input_lengths, self.txt_time, self.static = input_lengths, txt_time, static
        self.window_size, self.keep_bits, self.realtime = int(window_size), int(keep_bits), int(realtime)
        self.n_feat = bin(self.keep_bits).count("1")

    @property
    def batch_size(self) -> int:
        return int(self.input_lengths.numel())

    def descriptor(self) -> torch.Tensor:
        """int64 [B, 2]: (first_row, n_rows), the per-sample words of mtmp_hourly_window_gather."""
        return torch.from_numpy(np.ascontiguousarray(np.stack([self.first_row, self.n_rows], axis=1).astype(np.int64)))


class TieEventStore:
    """CSR form of all patients' hourly tables and events (module docstring).  The hour-level arrays live on the host (numpy) for
    ``plan``; ``to(device)`` uploads what the kernel reads, once."""

    def __init__(self, hour_ptr, present, norm, delta, hour_min, ev_ptr, ev_time, ev_val, ev_feat, static, names=None):
        self.hour_ptr, self.present, self.norm, self.delta, self.hour_min = hour_ptr, present, norm, delta, hour_min
        self.ev_ptr, self.static, self.names = ev_ptr, static, names
        # the events stay torch tensors: after to(device) no copy of them is kept on the host
        self.ev_time, self.ev_val, self.ev_feat = ev_time, ev_val, ev_feat
        self.device = torch.device("cpu")
        self._dev = None

    # ------------------------------------------------------------------------------------------------------------ building
    @classmethod
    def from_patients(cls, patients: Sequence[dict], feature_mins, feature_maxs, names: Optional[Sequence[str]] = None):
        fmin, fmax = np.asarray(feature_mins, np.float64), np.asarray(feature_maxs, np.float64)
        rng = np.subtract(fmax, fmin)
        names = [str(n) for n in names] if names is not None else [str(i) for i in range(len(patients))]
        hour_ptr, present, norm, delta, hour_min, ev_counts, times, vals, feats, static = [0], [], [], [], [], [], [], [], [], []
        for name, p in zip(names, patients):
            dit = p["data_in_time"]
            data = np.asarray(p["data"], np.float64).reshape(-1, N_FEAT)
            dl = np.asarray(p["delta"], np.float64).reshape(-1, N_FEAT)
            if not (data.shape[0] == dl.shape[0] == len(dit)):
                raise ValueError(f"patient {name}: data has {data.shape[0]} hours, delta {dl.shape[0]}, data_in_time {len(dit)}")
            norm.append(np.divide(np.subtract(data, fmin), rng).astype(np.float32))     # tie_window's expression, then its cast
            delta.append(dl)
            hour_ptr.append(hour_ptr[-1] + len(dit))
            for h, a in enumerate(dit):
                present.append(a is not None)
                ev = np.zeros((0, 3)) if a is None else np.asarray(a, np.float64).reshape(-1, 3)
                if not np.isfinite(ev[:, 0]).all():
                    raise ValueError(f"patient {name}: hour {h} holds a non-finite event time")
                f8 = ev[:, 2].astype(np.float32)
                with np.errstate(invalid="ignore"):
                    u8 = np.nan_to_num(f8, nan=0.0, posinf=0.0, neginf=0.0).clip(0, 255).astype(np.uint8)
                if not np.array_equal(u8.astype(np.float32).view(np.uint32), f8.view(np.uint32)):
                    raise ValueError(f"patient {name}: hour {h} holds a feature index that is not an integer 0..255")
                ev_counts.append(ev.shape[0])
                hour_min.append(ev[:, 0].min() if ev.shape[0] else np.inf)
                times.append(ev[:, 0])
                vals.append(ev[:, 1].astype(np.float32))
                feats.append(u8)
            static.append([1.0 if p["gender"] == "M" else 0.0, p["age"]])
        cat = lambda xs, dt, tail=(): np.concatenate(xs, axis=0).astype(dt, copy=False) if xs else np.zeros((0,) + tail, dt)
        ev_ptr = np.zeros(len(ev_counts) + 1, np.int64)
        np.cumsum(np.asarray(ev_counts, np.int64), out=ev_ptr[1:])
        return cls(np.asarray(hour_ptr, np.int64), np.asarray(present, bool), cat(norm, np.float32, (N_FEAT,)),
                   cat(delta, np.float64, (N_FEAT,)), np.asarray(hour_min, np.float64), ev_ptr,
                   torch.from_numpy(cat(times, np.float64)), torch.from_numpy(cat(vals, np.float32)),
                   torch.from_numpy(cat(feats, np.uint8)), np.asarray(static, np.float32).reshape(-1, 2), names)

    @classmethod
    def from_directory(cls, path: str, feature_mins, feature_maxs):
        """The pickles ``SampleTieDataset`` reads, in its (sorted) order."""
        files = sorted(glob.glob(os.path.join(path, "*.pkl")))
        if not files:
            raise FileNotFoundError(f"no *.pkl under {path}")
        patients = []
        for f in files:
            with open(f, "rb") as fh:
                p = pickle.load(fh)
            patients.append({k: p[k] for k in ("data", "delta", "data_in_time", "age", "gender")})
        return cls.from_patients(patients, feature_mins, feature_maxs, [os.path.basename(f) for f in files])

    # ------------------------------------------------------------------------------------------------------------ placement
    @property
    def n_patients(self) -> int:
        return int(self.hour_ptr.shape[0] - 1)

    @property
    def n_hours(self) -> int:
        return int(self.present.shape[0])

    @property
    def n_events(self) -> int:
        return int(self.ev_ptr[-1])

    @property
    def nbytes_hours(self) -> int:
        """bytes of what the kernel reads per patient-hour (norm, delta, hour_min; ev_ptr stays on the host: the plan resolves
        the event offsets)"""
        return int(self.norm.nbytes + self.delta.nbytes + self.hour_min.nbytes)

    @property
    def nbytes_events(self) -> int:
        return int(sum(t.numel() * t.element_size() for t in (self.ev_time, self.ev_val, self.ev_feat)))

    @property
    def nbytes(self) -> int:
        """size of the store as uploaded (the hour-level arrays the host keeps for ``plan`` are these same bytes again, plus
        ``present``, ``hour_ptr``, ``ev_ptr`` and ``static``)"""
        return self.nbytes_hours + self.nbytes_events

    def to(self, device):
        """Upload once.  The events move (no host copy is kept); the hour-level arrays stay on the host as well."""
        device = resolve_device(device)
        if device.type == "cpu" or device == self.device:
            return self
        self.ev_time, self.ev_val, self.ev_feat = (t.to(device) for t in (self.ev_time, self.ev_val, self.ev_feat))
        self._dev = dict(norm=torch.from_numpy(self.norm).to(device), delta=torch.from_numpy(self.delta).to(device),
                         hour_min=torch.from_numpy(self.hour_min).to(device))
        self.device = self.ev_time.device
        return self

    def device_arrays(self):
        if self._dev is None:
            raise RuntimeError("TieEventStore: call store.to(device) before ops.tie_windows (the store is uploaded once)")
        return self._dev

    # ------------------------------------------------------------------------------------------------------------ the plan
    def _trim(self, windows, who: str, train_missing: bool, window_size: Optional[int] = None):
        """The checks and the ``None``-hour trimming shared by ``plan`` and ``plan_hourly``: ``tie_window``'s control flow on the
        hour-level arrays, vectorised over the batch.  Returns (w, refuse, base, first, early, late, L2, key2)."""
        w = np.asarray(windows)
        if w.ndim != 2 or w.shape[1] != 3 or w.shape[0] < 1 or w.dtype.kind not in "iu":
            raise ValueError(f"{who}: windows must be an integer array [B >= 1, 3], got {w.dtype} {w.shape}")
        w = w.astype(np.int64)
        pat, key, L = w[:, 0], w[:, 1], w[:, 2]

        def refuse(bad, why):
            if bad.any():
                b = int(np.flatnonzero(bad)[0])
                raise ValueError(f"{who}: window {b} (patient {int(pat[b])}, selected_key {int(key[b])}, rand_length {int(L[b])}) {why}")
        refuse((pat < 0) | (pat >= self.n_patients), f"names a patient outside 0..{self.n_patients - 1}")
        base = self.hour_ptr[pat]
        refuse((key < 0) | (key >= self.hour_ptr[pat + 1] - base), "names an hour the patient does not have")
        refuse(L < 1, "has rand_length < 1")
        refuse(L > key + 1, "has rand_length > selected_key + 1")
        if window_size is not None:
            refuse(L > window_size, f"has rand_length > window_size {window_size}")
        first = key - L + 1                                   # sequenceGenerator's row 0: from the UNtrimmed key and length
        j = np.arange(int(L.max()), dtype=np.int64)[None, :]
        inside = j < L[:, None]
        pres = self.present[np.where(inside, (base + first)[:, None] + j, 0)] & inside
        refuse(~pres.any(axis=1), "has no hour with a measurement (all None)")
        first_p = pres.argmax(axis=1)
        last_p = pres.shape[1] - 1 - pres[:, ::-1].argmax(axis=1)
        head_none = ~pres[:, 0]
        tail_none = ~pres[np.arange(len(L)), L - 1]
        early = np.where(head_none, first_p, 0)               # one side only: `if tdl[0] is None ... elif tdl[-1] is None`
        late = np.where(~head_none & tail_none, L - last_p - 1, 0)
        L2 = L - early
        key2 = key - late if train_missing else key.copy()
        return w, refuse, base, first, early, late, L2, key2

    def plan(self, windows, tie_len: int, realtime: int, train_missing: bool = True) -> TieWindowBatch:
        """``windows`` int [B, 3] = (patient, selected_key, rand_length) -> TieWindowBatch.  ``tie_window``'s control flow on the
        hour-level arrays, vectorised over the batch."""
        w, refuse, base, first, early, late, L2, key2 = self._trim(windows, "plan", train_missing)
        pat, key, L = w[:, 0], w[:, 1], w[:, 2]
        t0 = key2 - L2 + 1
        first_hour = base + first + early
        last_hour = base + key - late                         # tdl[early:-late]: `late` cuts the hours whatever train_missing is
        first_event = self.ev_ptr[first_hour]
        n_events = self.ev_ptr[last_hour + 1] - first_event
        init_hour = base + first
        t_init = -self.delta[init_hour] + (t0 + 1).astype(np.float64)[:, None]      # the float64 expression of tie_window
        keep = t_init != t0.astype(np.float64)[:, None]
        mask = (keep.astype(np.int64) << np.arange(N_FEAT, dtype=np.int64)[None, :]).sum(axis=1)
        n_rows = keep.sum(axis=1).astype(np.int64) + n_events
        refuse(n_rows == 0, "has no row (no initial feature survives and its hours hold no event)")
        lens = np.minimum(n_rows, int(tie_len))
        refuse(lens < 1, f"has no row under tie_len {tie_len}")
        cu = torch.zeros(len(L) + 1, dtype=torch.int32)
        cu[1:] = torch.from_numpy(lens).cumsum(0).to(torch.int32)
        txt_time = torch.from_numpy((-key2 if realtime == 1 else np.zeros_like(key2)).astype(np.float32))
        return TieWindowBatch(self, w, first_event, n_events, mask, init_hour, first_hour, last_hour - first_hour + 1, key2, t0,
                              first, torch.from_numpy(lens), cu, txt_time, torch.from_numpy(self.static[pat]), tie_len, realtime)


    def plan_hourly(self, windows, window_size: int = 24, keep=None, realtime: int = 1,
                    train_missing: bool = True) -> HourlyWindowBatch:
        """``windows`` int [B, 3] = (patient, selected_key, rand_length) -> HourlyWindowBatch: the carry-forward branch of the
        reference's loader (dataset_new.py:2006-2011).  Plane 0 of its result is ``norm[key - L + 1 : key + 1][:, keep]`` followed
        by zero rows, its length the UNtrimmed ``rand_length``; only the text time sees the ``None``-hour trimming (``key2``)."""
        bits = _keep_bits(keep)
        w, _, base, first, _, _, _, key2 = self._trim(windows, "plan_hourly", train_missing, int(window_size))
        pat, L = w[:, 0], w[:, 2]
        txt_time = torch.from_numpy((-key2 if realtime == 1 else np.zeros_like(key2)).astype(np.float32))
        return HourlyWindowBatch(self, w, base + first, L.copy(), torch.from_numpy(L.copy()), txt_time,
                                 torch.from_numpy(self.static[pat]), window_size, bits, realtime)


class StoreWindowDataset(torch.utils.data.Dataset):
    """One random window ``(patient, selected_key, rand_length)`` of patient ``index`` per item, drawn with the ``random.choice``
    sequence of ``SampleTieDataset.__getitem__`` (the end hour among the sorted keys, then the length).  Nothing else is read."""

    def __init__(self, store: TieEventStore, window_size: int = 24, windows: Optional[List[dict]] = None):
        self.store, self.window_size, self.windows = store, window_size, windows

    def __len__(self):
        return self.store.n_patients

    def _windows_of(self, index: int) -> dict:
        if self.windows is not None:
            return self.windows[index]
        a, b = int(self.store.hour_ptr[index]), int(self.store.hour_ptr[index + 1])
        return {k: range(1, min(k + 1, self.window_size) + 1) for k in np.flatnonzero(self.store.present[a:b]).tolist()}

    def __getitem__(self, index: int):
        win = self._windows_of(index)
        key = random.choice(sorted(win))
        length = random.choice(win[key])
        return np.array([index, key, length], np.int32)          # 12 bytes: all a loader worker hands over


class StoreWindowSweep(torch.utils.data.Dataset):
    """EVERY window of the store as its own item, the way the reference's test data sets enumerate theirs (one item per
    (patient, hour), dataset_new.py:1113-1166, :2500-2553): item ``i`` is the ``i``-th ``(patient, key, length)`` over the patients
    in order and, inside a patient, over its present hours in order.  The length is ``min(key + 1, window_size)``; with
    ``windows`` (one dict per patient, hour -> the stored ``win_size`` of that hour, as the test data set's index files record
    it) the hours and the lengths are the list's."""

    def __init__(self, store: TieEventStore, window_size: int = 24, windows: Optional[List[dict]] = None):
        self.store, self.window_size = store, window_size
        if windows is not None:
            if len(windows) != store.n_patients:
                raise ValueError(f"StoreWindowSweep: {len(windows)} window lists for {store.n_patients} patients")
            items = [(p, int(k), int(w[k])) for p, w in enumerate(windows) for k in sorted(w)]
        else:
            items = []
            for p in range(store.n_patients):
                a, b = int(store.hour_ptr[p]), int(store.hour_ptr[p + 1])
                items += [(p, k, min(k + 1, window_size)) for k in np.flatnonzero(store.present[a:b]).tolist()]
        self.items = np.asarray(items, np.int32).reshape(-1, 3)

    def __len__(self):
        return self.items.shape[0]

    def __getitem__(self, index: int):
        return self.items[index].copy()                          # 12 bytes, like StoreWindowDataset's


def collate_windows(samples, store: TieEventStore, tie_len: int = 1000, realtime: int = 1,
                    train_missing: bool = True) -> TieWindowBatch:
    """Stacks the triples of ``StoreWindowDataset`` and plans the batch (as a DataLoader ``collate_fn``:
    ``functools.partial(collate_windows, store=store, tie_len=..., realtime=...)``)."""
    return store.plan(np.stack([np.asarray(s, np.int64).reshape(3) for s in samples]), tie_len, realtime, train_missing)


def collate_hourly_windows(samples, store: TieEventStore, window_size: int = 24, keep=None, realtime: int = 1,
                           train_missing: bool = True) -> HourlyWindowBatch:
    """The ``collate_fn`` twin of ``collate_windows`` for ``--vslt-type carryforward``: stacks the triples and plans the batch."""
    return store.plan_hourly(np.stack([np.asarray(s, np.int64).reshape(3) for s in samples]), window_size, keep, realtime,
                             train_missing)
