"""Device-resident training data: the encoded dataset lives in HBM and every batch is gathered on the GPU.

`LatentDataModule` (data.py) opens `<map>.latent.npz` and the mapset's `h.npy` for every map, every epoch — `h.npy` once per difficulty of
the same mapset — collates and zero-pads on the host, pins and copies.  Here every file is read ONCE into a flat fp32 device store
(`ResidentLatentStore`: `h` once per mapset, `z` per map, `s` / `labels` as tables), an epoch is planned on the host from the maps' lengths
alone (`EpochPlanner`: integers only), and a batch is built by `od_feed_gather` (csrc/misc.hip) from three small descriptor vectors that go
up in one stream-ordered copy: no loader workers, no per-epoch file reads, no host collate, no host-to-device copy of the batch.

Memory: a map of L latent frames takes 4 (A L / maps-in-its-mapset + E L + S + 5) bytes — 0.8 MB at L = 1500 and the default widths (A 128,
E 6) — so tens of thousands of maps fit in an MI355X's 288 GB beside the model; `max_bytes` (YAML: data.resident_max_gb) refuses a store
that would not, before anything is allocated.

The feed follows the host loader's rules in its three modes (an integer seq_len: fixed windows; seq_len None with batch_size N: N whole
maps per batch; batch_frames: frame-budget batches cut by data.cut_batches), with one difference that comes with planning a whole epoch at
once: the order is a full permutation of the epoch's samples instead of a shuffle buffer's, so `shuffle_buffer_size` has no meaning here.
With `data.resident_val` the denoiser's held-out maps live in a second store too and are validated in groups of whole maps
(`ResidentLatentValFeed`): every map cut into the trainer's val_batches segments by the same gather, one ragged no-grad forward per group,
and od_loss_finalize_groups for each map's own means.

The latent model's trainer has the same feed over the pre-processed beatmaps (the second half of this file): `BeatmapDataModule` opens the
mapset's whole `spec.npy` and the map's npz for every sample of every epoch, widens both to float64 and keeps one window.  Here
`ResidentBeatmapStore` keeps the files' unsigned integers on the device (spec once per mapset, hit and xy per map), the same `EpochPlanner`
plans the windows, `ResidentBeatmapFeed` draws their flips, and `od_feed_gather_quant` dequantises, places, flips and pads a batch in three
launches — bit for bit the host loader's float32 values.  With `data.resident_val` the held-out maps live in a second store and are
validated whole, in ragged groups (`ResidentBeatmapValFeed`): the same gather, then `od_replicate_tail` for the padding `pad_batch` applies.
"""
from __future__ import annotations

import zipfile
from pathlib import Path
from typing import Iterator, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from .data import (A_DIM, NUM_LABELS, X_DIM, Batch, BeatmapDataModule, BeatmapDataset, LatentBatch, LatentDataModule, LatentDataset,
                   RaggedBeatmapBatch, RaggedLatentBatch, RaggedLatentValBatch, _roundup, cut_batches)

ALL_FIELDS = ("h", "z", "s", "labels")
STYLE_FIELDS = ("s", "labels")


def _read_header(f) -> Tuple[Tuple[int, ...], np.dtype]:
    version = np.lib.format.read_magic(f)
    read = np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0
    shape, _, dtype = read(f)
    return tuple(int(x) for x in shape), np.dtype(dtype)


def npz_member_header(path, member: str) -> Tuple[Tuple[int, ...], np.dtype]:
    """(shape, dtype) of `member` of an .npz, from the member's .npy header (the array is not read)."""
    with zipfile.ZipFile(path) as z, z.open(member + ".npy") as f:
        return _read_header(f)


def npy_header(path) -> Tuple[Tuple[int, ...], np.dtype]:
    """(shape, dtype) of an .npy file, from its header (the array is not read or mapped)."""
    with open(path, "rb") as f:
        return _read_header(f)


def shard_files(mapsets: Sequence[Path], rank: int = 0, world_size: int = 1) -> List[Path]:
    """The rank's share of the dataset: files in `LatentDataset._files()` order, file i to rank i % world_size (the host loader's rank shard)."""
    return [f for i, f in enumerate(LatentDataset(list(mapsets))._files()) if i % world_size == rank]


# ------------------------------------------------------------------------------------------------------------------------------ the plan
class PlanBatch(NamedTuple):
    """One batch of an epoch plan, host integers only: row i takes frames starts[i] .. starts[i] + lens[i] of map maps[i] (an index into the
    store's files); Lpad is the batch's padded length (= seq_len for fixed windows).  The beatmap feed adds each window's flip
    augmentation: bit FLIP_X / FLIP_Y of flips[i] set = cursor x / y of row i is mirrored (v <- 1 - v), each with probability 1/2
    (BeatmapDataset.make_samples)."""
    maps: np.ndarray       # (B,) int64
    starts: np.ndarray     # (B,) int64
    lens: np.ndarray       # (B,) int64
    Lpad: int
    flips: Optional[np.ndarray] = None     # (B,) int32


class EpochPlanner:
    """Plans one epoch from the maps' lengths.  The three modes and their rules are LatentDataset.make_samples' and LatentDataModule's:

      * integer `seq_len`: per map, end = L - seq_len + 1 (maps with end < 1 contribute none), start = randint(0, min(seq_len, end)), windows at
        start, start + seq_len, ... < end, a random subset of at most `max_per_map` of them; all of the epoch's windows are permuted and cut into
        batches of `batch_size`, the last partial batch dropped (drop_last=True);
      * `seq_len` None, `batch_size` N: a permutation of the maps in chunks of N, a map longer than `max_len` contributing a random window of
        max_len frames, Lpad = the chunk's longest rounded up to `pad_multiple`; the last partial chunk is dropped;
      * `batch_frames`: pools of `bucket_pool` consecutive maps of the permutation go through data.cut_batches, each pool's batches are
        shuffled, and the partial last pool is cut too: no map is dropped.
    """

    def __init__(self, lengths: Sequence[int], batch_size: int, seq_len: Optional[int], max_per_map: int = -1, max_len: Optional[int] = None,
                 pad_multiple: int = 64, batch_frames: Optional[int] = None, bucket_pool: Optional[int] = None):
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.batch_size, self.seq_len = int(batch_size), seq_len
        self.max_per_map = int(max_per_map) if max_per_map > 0 else None
        self.max_len, self.pad_multiple = max_len, int(pad_multiple)
        self.batch_frames = batch_frames
        self.bucket_pool = (64 * self.batch_size if bucket_pool is None else int(bucket_pool)) if batch_frames is not None else None

    def plan(self, gen: torch.Generator) -> List[PlanBatch]:
        if self.seq_len is not None:
            return self._windows(gen)
        return self._bucketed(gen) if self.batch_frames is not None else self._chunks(gen)

    # ---- fixed windows
    def _windows(self, gen) -> List[PlanBatch]:
        T = int(self.seq_len)
        end = self.lengths - T + 1
        live = np.nonzero(end >= 1)[0]
        if len(live) == 0:
            return []
        end = end[live]
        hi = np.minimum(T, end)
        start = np.minimum((torch.rand(len(live), generator=gen, dtype=torch.float64).numpy() * hi).astype(np.int64), hi - 1)
        count = (end - start + T - 1) // T                      # len(arange(start, end, T)) >= 1
        maps, starts = [], []
        if self.max_per_map == 1:                               # the shipped configs: one random window per map, no per-map loop
            pick = np.minimum((torch.rand(len(live), generator=gen, dtype=torch.float64).numpy() * count).astype(np.int64), count - 1)
            maps, starts = [live], [start + pick * T]
        else:
            for m, s0, k in zip(live.tolist(), start.tolist(), count.tolist()):
                idx = np.arange(k, dtype=np.int64)
                if self.max_per_map is not None and k > self.max_per_map:
                    idx = torch.randperm(k, generator=gen)[:self.max_per_map].numpy()
                maps.append(np.full(len(idx), m, dtype=np.int64))
                starts.append(s0 + idx * T)
        maps, starts = np.concatenate(maps), np.concatenate(starts)
        perm = torch.randperm(len(maps), generator=gen).numpy()
        maps, starts = maps[perm], starts[perm]
        B = self.batch_size
        lens = np.full(B, T, dtype=np.int64)
        return [PlanBatch(maps[i:i + B], starts[i:i + B], lens, T) for i in range(0, len(maps) - B + 1, B)]

    # ---- whole maps
    def _whole(self, gen) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """A permutation of the maps with each map's window: (maps, starts, lens)."""
        maps = torch.randperm(len(self.lengths), generator=gen).numpy()
        L = self.lengths[maps]
        starts, lens = np.zeros_like(L), L.copy()
        if self.max_len is not None:
            over = L > self.max_len
            room = np.where(over, L - self.max_len + 1, 1)
            draw = np.minimum((torch.rand(len(maps), generator=gen, dtype=torch.float64).numpy() * room).astype(np.int64), room - 1)
            starts, lens = np.where(over, draw, 0), np.where(over, self.max_len, L)
        return maps, starts, lens

    def _batch(self, maps, starts, lens) -> PlanBatch:
        return PlanBatch(maps, starts, lens, _roundup(int(lens.max()), self.pad_multiple))

    def _chunks(self, gen) -> List[PlanBatch]:
        maps, starts, lens = self._whole(gen)
        N = self.batch_size
        return [self._batch(maps[i:i + N], starts[i:i + N], lens[i:i + N]) for i in range(0, len(maps) - N + 1, N)]

    def _bucketed(self, gen) -> List[PlanBatch]:
        maps, starts, lens = self._whole(gen)
        out: List[PlanBatch] = []
        for p in range(0, len(maps), self.bucket_pool):
            sl = slice(p, p + self.bucket_pool)
            groups = cut_batches(lens[sl].tolist(), self.batch_frames, self.batch_size, self.pad_multiple)
            for gi in torch.randperm(len(groups), generator=gen).tolist():
                g = np.asarray(groups[gi], dtype=np.int64) + p
                out.append(self._batch(maps[g], starts[g], lens[g]))
        return out


# ----------------------------------------------------------------------------------------------------------------------------- the store
def _refuse_over_limit(nbytes: int, n: int, max_bytes: Optional[int], reserved_bytes: int = 0):
    """MemoryError for a store of `nbytes` for `n` maps that does not fit under `max_bytes` beside the `reserved_bytes` another store under
    the same limit already holds.  The stores call it with sizes read from headers: before anything is allocated or any array read."""
    if max_bytes is None or nbytes + reserved_bytes <= max_bytes:
        return
    limit = f"the limit of {int(max_bytes)} bytes (data.resident_max_gb = {max_bytes / 2 ** 30:.2f}): raise the limit, or "
    if reserved_bytes:
        raise MemoryError(f"the resident store of the held-out maps needs {nbytes} bytes for {n} maps beside the training store's "
                          f"{int(reserved_bytes)}: together more than {limit}validate with data.resident_val: false")
    raise MemoryError(f"the resident store needs {nbytes} bytes ({nbytes / 2 ** 30:.2f} GiB) for {n} maps, more than {limit}train with "
                      "data.resident: false")


def _device_or_default(device) -> torch.device:
    return torch.device(device) if device is not None else _lib.training_device(None, "data.resident")


def _gb_to_bytes(gb: Optional[float]) -> Optional[int]:
    return None if gb is None else int(float(gb) * 2 ** 30)


class ResidentLatentStore:
    """The rank's share of an encoded dataset on `device`, every file read once.

      data     flat fp32: every mapset's `h` (A, Lh) once, then every map's `z` (E, L), each array as it lies in its file (channel-major);
               h_base / h_stride / z_base / lengths (host int64, one per map) locate them: channel c of map m's h starts at
               h_base[m] + c * h_stride[m] (maps of one mapset share the values), of its z at z_base[m] + c * lengths[m]
      s        (n_maps, S) fp32,  labels (n_maps, 5) fp32: tables for torch.index_select
      lengths  latent frames per map (z's), on the host: all an epoch plan needs

    `fields` without "h" / "z" (the style model's feed) reads the `s` and `labels` members only and never opens h.npy; the lengths then
    come from the header of the `z` member (its array is not read).  The upload goes through two pinned staging buffers of `staging_bytes`
    each, not through a host copy of the dataset.  `max_bytes`: refuse — before anything is allocated — a store that needs more, counting
    `reserved_bytes` that another store under the same limit already holds."""

    def __init__(self, mapsets: Sequence[Path], device, fields: Sequence[str] = ALL_FIELDS, rank: int = 0, world_size: int = 1,
                 max_bytes: Optional[int] = None, staging_bytes: int = 32 << 20, reserved_bytes: int = 0):
        self.device = torch.device(device)
        self.fields = tuple(fields)
        if not set(self.fields) <= set(ALL_FIELDS) or not {"s", "labels"} <= set(self.fields) or ("h" in self.fields) != ("z" in self.fields):
            raise ValueError(f"fields must be {ALL_FIELDS} or {STYLE_FIELDS}, got {self.fields}")
        self.has_frames = "h" in self.fields
        self.files = shard_files(mapsets, rank, world_size)
        if not self.files:
            raise ValueError(f"no *.latent.npz file for rank {rank} of {world_size}")
        # ---- sizes from the headers
        z_shapes = [npz_member_header(f, "z")[0] for f in self.files]
        self.lengths = np.asarray([sh[-1] for sh in z_shapes], dtype=np.int64)
        self.style_dim = int(np.prod(npz_member_header(self.files[0], "s")[0]))
        self.emb_dim = int(z_shapes[0][0])
        n = len(self.files)
        self.h_base, self.h_stride = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        self.z_base = np.zeros(n, dtype=np.int64)
        self.a_dim = 0
        h_files: List[Tuple[Path, int]] = []                   # (mapset's h.npy, its offset), each once
        elems = 0
        if self.has_frames:
            seen = {}
            for i, f in enumerate(self.files):
                d = f.parent
                if d not in seen:
                    A, Lh = npy_header(d / "h.npy")[0]
                    self.a_dim = self.a_dim or A
                    if A != self.a_dim:
                        raise ValueError(f"{d / 'h.npy'}: {A} channels, the dataset's other maps have {self.a_dim}")
                    seen[d] = (elems, Lh)
                    h_files.append((d / "h.npy", elems))
                    elems += A * Lh
                self.h_base[i], self.h_stride[i] = seen[d]
                if z_shapes[i][0] != self.emb_dim or self.h_stride[i] < self.lengths[i]:
                    raise ValueError(f"{f}: z {z_shapes[i]} does not fit the dataset (emb_dim {self.emb_dim}) or its mapset's h ({self.h_stride[i]} frames)")
            for i in range(n):
                self.z_base[i] = elems
                elems += self.emb_dim * int(self.lengths[i])
        self.nbytes = 4 * (elems + n * (self.style_dim + NUM_LABELS))
        _refuse_over_limit(self.nbytes, n, max_bytes, reserved_bytes)
        # ---- allocate and fill
        self.data = torch.empty(max(elems, 1), dtype=torch.float32, device=self.device)
        s_host, labels_host = np.empty((n, self.style_dim), dtype=np.float32), np.empty((n, NUM_LABELS), dtype=np.float32)
        up = _Uploader(self.device, staging_bytes)
        for path, off in h_files:
            up.put(self.data, off, np.load(path))
        for i, f in enumerate(self.files):
            with np.load(f) as d:
                s_host[i], labels_host[i] = d["s"].reshape(-1), d["labels"].reshape(-1)
                if self.has_frames:
                    up.put(self.data, int(self.z_base[i]), d["z"])
        up.finish()
        self.s = torch.from_numpy(s_host).to(self.device)
        self.labels = torch.from_numpy(labels_host).to(self.device)

    def __len__(self):
        return len(self.files)


class _Uploader:
    """Host arrays -> slices of a flat device tensor of `dtype` through two pinned staging buffers used in turn (a buffer is refilled only
    after the copy that read it has finished).  On the host (the test-suite's emulator backend) a plain copy."""

    def __init__(self, device, staging_bytes: int, dtype: torch.dtype = torch.float32):
        self.cuda = device.type == "cuda"
        self.np_dtype = torch.empty(0, dtype=dtype).numpy().dtype
        if self.cuda:
            k = max(1, staging_bytes // self.np_dtype.itemsize)
            self.bufs = [torch.empty(k, dtype=dtype, pin_memory=True) for _ in range(2)]
            self.events = [None, None]
            self.turn = 0
            self.stream = torch.cuda.current_stream(device)

    def put(self, dst: torch.Tensor, off: int, arr: np.ndarray):
        flat = np.ascontiguousarray(arr, dtype=self.np_dtype).reshape(-1)
        if not self.cuda:
            dst[off:off + flat.size].copy_(torch.from_numpy(flat))
            return
        k = self.bufs[0].numel()
        for i in range(0, flat.size, k):
            b = self.turn
            self.turn ^= 1
            if self.events[b] is not None:
                self.events[b].synchronize()
            m = min(k, flat.size - i)
            self.bufs[b].numpy()[:m] = flat[i:i + m]
            dst[off + i:off + i + m].copy_(self.bufs[b][:m], non_blocking=True)
            self.events[b] = torch.cuda.Event()
            self.events[b].record(self.stream)

    def finish(self):
        if self.cuda:
            self.stream.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------ the feed
def pack_descriptors(device, pin: bool, i64: Sequence[np.ndarray] = (), f64: Sequence[np.ndarray] = (), i32: Sequence[np.ndarray] = ()):
    """The device views of a batch's host columns, in the order given, behind ONE stream-ordered copy: the columns fill one host block
    (pinned when `pin`) — the 8-byte ones first, so that every fp64 view stays 8-byte aligned, the int32 ones behind them — and one
    device block takes it.  A view has its column's shape.  The pinned block returns to torch's host allocator, which hands it out again
    only after that copy has run."""
    n8, n4 = 0, 0                                   # plain loops throughout: this runs per batch, on a launch-bound path
    for c in i64:
        n8 += c.size
    for c in f64:
        n8 += c.size
    for c in i32:
        n4 += c.size
    host = torch.empty(n8 + (n4 + 1) // 2, dtype=torch.int64, pin_memory=pin)
    hv = host.numpy()
    desc = torch.empty(host.numel(), dtype=torch.int64, device=device)
    views, o = [], 0
    for c in i64:
        e = o + c.size
        hv[o:e] = c
        views.append(desc[o:e])
        o = e
    for c in f64:
        e = o + c.size
        hv[o:e].view(np.float64)[:] = c.reshape(-1)
        views.append(desc[o:e].view(torch.float64).view(c.shape))
        o = e
    if i32:
        h32, d32, o = hv[n8:].view(np.int32), desc[n8:].view(torch.int32), 0
        for c in i32:
            e = o + c.size
            h32[o:e] = c
            views.append(d32[o:e])
            o = e
    desc.copy_(host, non_blocking=True)
    return views


def _assert_inside_maps(map_lens: np.ndarray, starts: np.ndarray, lens: np.ndarray, Lpad: int):
    # a descriptor outside the store would be caught by the kernel (NaN rows); a plan that leaves its map is a bug to stop here
    assert (starts >= 0).all() and (lens >= 1).all() and (lens <= Lpad).all() and (starts + lens <= map_lens).all()


class _EpochFeed:
    """Re-iterable over the batches of one epoch each: every iter() draws a new plan from the feed's generator — seeded, at the first epoch,
    like the host datasets' __iter__ (torch.initial_seed() + 7919 * rank) — and yields the plan's batches, built on the device by gather()."""

    def __init__(self, store, planner: EpochPlanner, rank: int = 0):
        self.store, self.planner, self.rank = store, planner, rank
        self.gen: Optional[torch.Generator] = None
        self.pin = store.device.type == "cuda"

    def plan_epoch(self) -> List[PlanBatch]:
        if self.gen is None:
            self.gen = torch.Generator().manual_seed(torch.initial_seed() + 7919 * self.rank)
        return self.planner.plan(self.gen)

    def __iter__(self) -> Iterator:
        for pb in self.plan_epoch():
            yield self.gather(pb)


class ResidentFeed(_EpochFeed):
    """The feed of the encoded dataset (ResidentLatentStore): LatentBatch, or RaggedLatentBatch when `ragged`."""

    def __init__(self, store: ResidentLatentStore, planner: EpochPlanner, ragged: bool, rank: int = 0):
        super().__init__(store, planner, rank)
        self.ragged = ragged

    def gather(self, pb: PlanBatch):
        """The device batch of one plan entry: h and z by od_feed_gather, s and labels by index_select.  The descriptors (h base, h channel
        stride, z base, z channel stride, map index as int64, the lengths as int32) travel as one copy (pack_descriptors)."""
        st, B = self.store, len(pb.maps)
        if st.has_frames:
            map_lens = st.lengths[pb.maps]                      # z's channel stride
            _assert_inside_maps(map_lens, pb.starts, pb.lens, pb.Lpad)
            h_base, h_stride, z_base, z_stride, maps, lens32 = pack_descriptors(
                st.device, self.pin, i64=(st.h_base[pb.maps] + pb.starts, st.h_stride[pb.maps], st.z_base[pb.maps] + pb.starts, map_lens,
                                          pb.maps), i32=(pb.lens,))
            h = torch.empty(B, st.a_dim, pb.Lpad, dtype=torch.float32, device=st.device)
            z = torch.empty(B, st.emb_dim, pb.Lpad, dtype=torch.float32, device=st.device)
            ops.feed_gather(st.data, h_base, h_stride, lens32, h)
            ops.feed_gather(st.data, z_base, z_stride, lens32, z)
        else:
            maps, = pack_descriptors(st.device, self.pin, i64=(pb.maps,))
            h = torch.empty(B, 0, pb.Lpad, dtype=torch.float32, device=st.device)      # the style model reads s and labels only
            z = torch.empty(B, 0, pb.Lpad, dtype=torch.float32, device=st.device)
        s, labels = st.s.index_select(0, maps), st.labels.index_select(0, maps)
        if self.ragged:
            return RaggedLatentBatch(h, z, s, labels, torch.from_numpy(pb.lens.astype(np.int64)))
        return LatentBatch(h, z, s, labels)


DEFAULT_VAL_FRAME_BUDGET = 1 << 17     # padded frames of a validation group: half of a training step of 32 windows x 8192 frames


class ResidentLatentValFeed:
    """Re-iterable over one validation epoch of the held-out maps in `store`, whole maps in groups (`data.RaggedLatentValBatch`).

    `DiffusionTrainer.validation_step` cuts a map of L frames into `val_batches` segments of seg = L // val_batches frames and evaluates
    them as one batch.  The plan here is made once, from the store's lengths: the maps with seg >= 1 are packed longest first
    (encode_latents.pack) into groups whose padded size, val_batches x G x (the longest seg rounded up to `pad_multiple`), stays within
    `frame_budget`; a map over the budget goes alone.  A group is built by two od_feed_gather launches behind one descriptor copy: row
    val_batches * g + j takes seg_g frames from frame j * seg_g of map g's z and of its mapset's h — bit for bit the slices
    validation_step cuts from the host loader's tensors — and zeros behind them; s and labels come from index_select.

    A map of fewer than `val_batches` frames has seg = 0, no frame to evaluate: such maps are not grouped and follow the groups one by
    one as the host loader's batch-1 tuple (h, z, s, labels), which validation_step treats as it always has (it refuses a map without a
    frame per segment, from either loader).

    `limit(n)`: plan over the first n held-out maps of the host loader's order (the store's), which is what `limit_val_batches` means."""

    def __init__(self, store: ResidentLatentStore, val_batches: int, pad_multiple: int = 64, frame_budget: Optional[int] = None):
        if not store.has_frames:
            raise ValueError("the resident validation of the denoiser gathers h and z: the store must hold them (fields = ALL_FIELDS)")
        if val_batches < 1 or pad_multiple < 1:
            raise ValueError(f"invalid {val_batches=} / {pad_multiple=}")
        self.store, self.val_batches, self.pad_multiple = store, int(val_batches), int(pad_multiple)
        self.frame_budget = int(DEFAULT_VAL_FRAME_BUDGET if frame_budget is None else frame_budget)
        if self.frame_budget < 1:
            raise ValueError(f"data.val_frame_budget must be at least 1 frame, got {frame_budget}")
        self.segs = store.lengths // self.val_batches
        self.pin = store.device.type == "cuda"
        self.limit(None)

    def limit(self, n: Optional[int]) -> "ResidentLatentValFeed":
        """Plan over the first `n` maps of the store (None: all of them)."""
        from .encode_latents import pack
        self.count = len(self.store) if n is None else max(0, min(int(n), len(self.store)))
        first = np.arange(self.count)
        whole = first[self.segs[:self.count] >= 1]
        padded = self.val_batches * _roundup_all(self.segs[whole], self.pad_multiple)
        self.groups: List[np.ndarray] = [whole[g] for g in pack(padded.tolist(), self.frame_budget)]
        self.short: np.ndarray = first[self.segs[:self.count] < 1]
        return self

    def __len__(self):
        return len(self.groups) + len(self.short)

    def padded_share(self) -> List[float]:
        """Per group, the share of its R x Lpad frames that belong to no segment (zeros)."""
        vb = self.val_batches
        return [1.0 - float(vb * self.segs[g].sum()) / (vb * len(g) * _roundup(int(self.segs[g].max()), self.pad_multiple)) for g in self.groups]

    def gather(self, maps: np.ndarray) -> RaggedLatentValBatch:
        """The device batch of one group.  The descriptors (h base, h channel stride, z base, z channel stride per row, the map indices, the
        rows' lengths as int32) travel as one copy (pack_descriptors)."""
        st, vb = self.store, self.val_batches
        seg = self.segs[maps]
        Lpad = _roundup(int(seg.max()), self.pad_multiple)
        rows = np.repeat(maps, vb)
        lens = np.repeat(seg, vb)
        starts = np.tile(np.arange(vb, dtype=np.int64), len(maps)) * lens
        map_lens = st.lengths[rows]                             # z's channel stride
        _assert_inside_maps(map_lens, starts, lens, Lpad)
        h_base, h_stride, z_base, z_stride, idx, lens32 = pack_descriptors(
            st.device, self.pin, i64=(st.h_base[rows] + starts, st.h_stride[rows], st.z_base[rows] + starts, map_lens, maps), i32=(lens,))
        R = len(rows)
        h = torch.empty(R, st.a_dim, Lpad, dtype=torch.float32, device=st.device)
        z = torch.empty(R, st.emb_dim, Lpad, dtype=torch.float32, device=st.device)
        ops.feed_gather(st.data, h_base, h_stride, lens32, h)
        ops.feed_gather(st.data, z_base, z_stride, lens32, z)
        return RaggedLatentValBatch(h, z, st.s.index_select(0, idx), st.labels.index_select(0, idx), torch.from_numpy(lens.astype(np.int64)),
                                    torch.arange(0, R + 1, vb, dtype=torch.int64))

    def gather_one(self, m: int):
        """Map m whole, as the host loader's batch-1 tuple: (h (1, A, Lh) — the mapset's whole h — z (1, E, L), s (1, S), labels (1, 5))."""
        st = self.store
        Lh, L = int(st.h_stride[m]), int(st.lengths[m])
        h = st.data[int(st.h_base[m]):int(st.h_base[m]) + st.a_dim * Lh].view(1, st.a_dim, Lh)
        z = st.data[int(st.z_base[m]):int(st.z_base[m]) + st.emb_dim * L].view(1, st.emb_dim, L)
        return h, z, st.s[m:m + 1], st.labels[m:m + 1]

    def __iter__(self) -> Iterator:
        for g in self.groups:
            yield self.gather(g)
        for m in self.short.tolist():
            yield self.gather_one(m)


def _roundup_all(n: np.ndarray, m: int) -> np.ndarray:
    return (n + m - 1) // m * m


class ResidentLatentDataModule:
    """`LatentDataModule` with the training set resident on `device`: the same constructor keys (the YAML `data:` block) and the same three
    feed modes, plus `device`, `fields` (STYLE_FIELDS for fit-style: s and labels only), `resident_max_gb`, and `resident_val` with
    `val_frame_budget` and `val_batches`.  Unless `resident_val`, the denoiser's validation stays the host loader (whole maps read once
    per check), which is all `num_workers` still serves; `shuffle_buffer_size` serves nothing: an epoch is a full permutation.  With
    `resident_val` the held-out maps — all of them on every rank, as the host loader hands them out — go, on first use, into a second
    store under the same `resident_max_gb`, and validation reads groups of whole maps from it (ResidentLatentValFeed), each map cut into
    the trainer's `val_batches` segments (fit-denoiser passes the model's)."""

    def __init__(self, batch_size: int, seq_len: Optional[int], num_workers: int = 0, max_val_count: int = 512, max_val_frac: float = .3,
                 data_path: str = "./data", shuffle_buffer_size: int = 1, max_per_map: int = -1, rank: int = 0, world_size: int = 1,
                 max_len: Optional[int] = None, pad_multiple: int = 64, batch_frames: Optional[int] = None, bucket_pool: Optional[int] = None,
                 device=None, fields: Sequence[str] = ALL_FIELDS, resident_max_gb: Optional[float] = None, resident_val: bool = False,
                 val_frame_budget: Optional[int] = None, val_batches: Optional[int] = None):
        if resident_val and tuple(fields) != ALL_FIELDS:
            raise ValueError("data.resident_val validates the denoiser from h and z: a style-only store validates from its own table already")
        if resident_val and val_batches is None:
            raise ValueError("data.resident_val cuts every held-out map as the trainer does: val_batches (the model's) is needed")
        if val_frame_budget is not None and not resident_val:
            raise ValueError("data.val_frame_budget sizes the groups of the resident validation: set data.resident_val: true, or drop the key")
        # the host module validates the keys, holds out the validation mapsets and keeps the validation loader
        self.host = LatentDataModule(batch_size, seq_len, num_workers, max_val_count, max_val_frac, data_path, shuffle_buffer_size, max_per_map,
                                     rank, world_size, max_len, pad_multiple, batch_frames, bucket_pool)
        self.device, self.fields = _device_or_default(device), tuple(fields)
        self.ragged, self.rank = self.host.ragged, rank
        max_bytes = _gb_to_bytes(resident_max_gb)
        self.store = ResidentLatentStore(self.host.train_set.mapsets, self.device, self.fields, rank, world_size, max_bytes)
        self.planner = EpochPlanner(self.store.lengths, batch_size, seq_len, max_per_map, max_len, pad_multiple, self.host.batch_frames,
                                    self.host.bucket_pool)
        self.feed = ResidentFeed(self.store, self.planner, self.ragged, rank)
        self._val_store: Optional[ResidentLatentStore] = None
        self._max_bytes = max_bytes
        self.resident_val = bool(resident_val)
        self._val_args = (val_batches, self.host.pad_multiple, val_frame_budget)
        self.val_feed: Optional[ResidentLatentValFeed] = None

    def train_dataloader(self) -> ResidentFeed:
        return self.feed

    def val_dataloader(self):
        if self.resident_val:
            if self.val_feed is None:
                # refused, before anything is allocated, if it does not fit under resident_max_gb beside the training store
                val_store = ResidentLatentStore(self.host.val_set.mapsets, self.device, max_bytes=self._max_bytes, reserved_bytes=self.store.nbytes)
                self.val_feed = ResidentLatentValFeed(val_store, *self._val_args)
            return self.val_feed
        if self.store.has_frames:
            return self.host.val_dataloader()
        return self._style_val()

    def _style_val(self) -> Iterator:
        """Batch-1 tuples (empty h, empty z, s (1, S), labels (1, 5)) over the held-out maps, from a style store of their own."""
        if self._val_store is None:
            self._val_store = ResidentLatentStore(self.host.val_set.mapsets, self.device, STYLE_FIELDS, max_bytes=self._max_bytes)
        vs = self._val_store
        empty = torch.empty(1, 0, 1, dtype=torch.float32, device=self.device)
        for i in range(len(vs)):
            yield empty, empty, vs.s[i:i + 1], vs.labels[i:i + 1]


# ------------------------------------------------------------------------------------------- the latent model's feed: quantised beatmaps
HIT_DIM = X_DIM - 2                    # chart rows 0..6 come from `hit` (uint8), rows 7, 8 (cursor x, y) from `xy` (uint16)
FLIP_X, FLIP_Y = 1, 2                  # bits of a window's flip mask = bits of od_feed_gather_quant's mask over the two xy channels


class ResidentBeatmapStore:
    """The rank's share of a pre-processed beatmap dataset on `device`, every file read once and kept AS STORED — unsigned integers:

      data      flat uint8: every mapset's `spec.npy` (72, Ls) once, then every map's `hit` (7, L), then every map's `xy` (2, L) uint16 at a
                4-byte-aligned byte offset, each array as it lies in its file (channel-major)
      spec_base / spec_stride / hit_base / xy_base / lengths  (host int64, one per map): channel c of map m's spectrogram starts at byte
                spec_base[m] + c * spec_stride[m] (maps of one mapset share the values), of its hit at byte hit_base[m] + c * lengths[m], of
                its xy at uint16 ELEMENT xy_base[m] + c * lengths[m]
      xy_rng / xy_min  (n_maps, 2) fp64 on the host: they travel with each batch's descriptors (od_feed_gather_quant's scale / offset)
      labels    (n_maps, 5) fp32 on the device: a table for torch.index_select
      lengths   chart frames per map, on the host: all an epoch plan needs

    A 30 000-frame mapset takes 2.2 MB plus 0.33 MB per difficulty: 11 bytes per chart frame against the 324 a float32 batch spends.
    Every size and dtype is read from the files' headers first; `max_bytes`: refuse — before anything is allocated — a store that needs
    more, counting `reserved_bytes` that another store under the same limit already holds.  The upload goes through two pinned staging
    buffers of `staging_bytes` each."""

    def __init__(self, mapsets: Sequence[Path], device, rank: int = 0, world_size: int = 1, max_bytes: Optional[int] = None,
                 staging_bytes: int = 32 << 20, reserved_bytes: int = 0):
        self.device = torch.device(device)
        self.files = [f for i, f in enumerate(BeatmapDataset(list(mapsets))._files()) if i % world_size == rank]
        if not self.files:
            raise ValueError(f"no *.map.npy file for rank {rank} of {world_size}")
        n = len(self.files)
        # ---- sizes and dtypes from the headers
        self.lengths = np.zeros(n, dtype=np.int64)
        self.spec_base, self.spec_stride = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        self.hit_base, self.xy_base = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        spec_files: List[Tuple[Path, int]] = []                # (mapset's spec.npy, its byte offset), each once
        seen = {}
        nbytes = 0
        for i, f in enumerate(self.files):
            (hit_shape, hit_dt), (xy_shape, xy_dt) = npz_member_header(f, "hit"), npz_member_header(f, "xy")
            if hit_dt != np.uint8 or xy_dt != np.uint16:
                raise ValueError(f"{f}: hit is {hit_dt} and xy is {xy_dt}; the resident store keeps hit as uint8 and xy as uint16, as the "
                                 "pre-processing writes them")
            L = hit_shape[-1]
            if hit_shape != (HIT_DIM, L) or xy_shape != (2, L):
                raise ValueError(f"{f}: hit {hit_shape} / xy {xy_shape}, expected ({HIT_DIM}, L) / (2, L)")
            self.lengths[i] = L
            d = f.parent
            if d not in seen:
                spec = d / "spec.npy"
                shape, dt = npy_header(spec)
                if dt != np.uint8:
                    raise ValueError(f"{spec}: dtype {dt}; the resident store keeps spectrograms as uint8, as the pre-processing writes them")
                if len(shape) != 2 or shape[0] != A_DIM:
                    raise ValueError(f"{spec}: shape {shape}, expected ({A_DIM}, frames)")
                seen[d] = (nbytes, shape[1])
                spec_files.append((spec, nbytes))
                nbytes += A_DIM * shape[1]
            self.spec_base[i], self.spec_stride[i] = seen[d]
            if self.spec_stride[i] < L:
                raise ValueError(f"{d / 'spec.npy'}: {self.spec_stride[i]} frames, shorter than its map {f.name} ({L} frames)")
        for i in range(n):
            self.hit_base[i] = nbytes
            nbytes += HIT_DIM * int(self.lengths[i])
        for i in range(n):
            nbytes = _roundup(nbytes, 4)
            self.xy_base[i] = nbytes // 2
            nbytes += 2 * 2 * int(self.lengths[i])
        self.nbytes = nbytes + 4 * n * NUM_LABELS
        _refuse_over_limit(self.nbytes, n, max_bytes, reserved_bytes)
        # ---- allocate and fill
        self.data = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.xy_rng, self.xy_min = np.empty((n, 2), dtype=np.float64), np.empty((n, 2), dtype=np.float64)
        labels_host = np.empty((n, NUM_LABELS), dtype=np.float32)
        up = _Uploader(self.device, staging_bytes, torch.uint8)
        for path, off in spec_files:
            up.put(self.data, off, np.load(path))
        for i, f in enumerate(self.files):
            with np.load(f) as d:
                up.put(self.data, int(self.hit_base[i]), d["hit"])
                up.put(self.data, 2 * int(self.xy_base[i]), np.ascontiguousarray(d["xy"]).view(np.uint8))
                self.xy_rng[i], self.xy_min[i] = np.asarray(d["xy_rng"], dtype=np.float64).reshape(2), np.asarray(d["xy_min"], dtype=np.float64).reshape(2)
                labels_host[i] = np.asarray(d["labels"]).reshape(-1)
        up.finish()
        self.labels = torch.from_numpy(labels_host).to(self.device)

    def __len__(self):
        return len(self.files)


def gather_beatmap_rows(st: ResidentBeatmapStore, pin: bool, maps: np.ndarray, starts: np.ndarray, lens: np.ndarray, Lpad: int,
                        aux: np.ndarray, flip: bool):
    """(audio (B, 72, Lpad), chart (B, 9, Lpad), the maps' indices, lens and aux as device int32): row i takes lens[i] frames of map
    maps[i] from frame starts[i], zeros behind.  Everything the three od_feed_gather_quant launches read per row travels as one copy
    (pack_descriptors), 11 B 64-bit words: the spectrogram's base and channel stride, the hit and xy bases, the chart's channel stride,
    the map index (for the labels), xy_rng and xy_min as fp64 (B, 2) each, then the lengths and `aux` as int32.
    `aux` (B,) is the rows' flip masks when `flip`, else whatever int32 the caller wants on the device beside the lengths."""
    B = len(maps)
    map_lens = st.lengths[maps]                                 # the chart's channel stride
    _assert_inside_maps(map_lens, starts, lens, Lpad)
    spec_base, spec_stride, hit_base, xy_base, stride, idx, rng, lo, lens32, aux32 = pack_descriptors(
        st.device, pin, i64=(st.spec_base[maps] + starts, st.spec_stride[maps], st.hit_base[maps] + starts, st.xy_base[maps] + starts,
                             map_lens, maps), f64=(st.xy_rng[maps], st.xy_min[maps]), i32=(lens, aux))
    audio = torch.empty(B, A_DIM, Lpad, dtype=torch.float32, device=st.device)
    chart = torch.empty(B, X_DIM, Lpad, dtype=torch.float32, device=st.device)
    ops.feed_gather_quant(st.data, 1, spec_base, spec_stride, lens32, audio)
    ops.feed_gather_quant(st.data, 1, hit_base, stride, lens32, chart, c0=0, channels=HIT_DIM)
    ops.feed_gather_quant(st.data, 2, xy_base, stride, lens32, chart, c0=HIT_DIM, channels=2, scale=rng, offset=lo,
                          flip=aux32 if flip else None)
    return audio, chart, idx, lens32, aux32


class ResidentBeatmapFeed(_EpochFeed):
    """The feed of the pre-processed beatmaps (ResidentBeatmapStore): the windows by EpochPlanner's fixed-window rule on the chart lengths
    (BeatmapDataset.make_samples' rule), then the two flips of every window, and `data.Batch`es built on the device by three
    od_feed_gather_quant launches."""

    def __init__(self, store: ResidentBeatmapStore, planner: EpochPlanner, rank: int = 0):
        if planner.seq_len is None:
            raise ValueError("the resident beatmap feed cuts fixed windows: it needs an integer seq_len")
        super().__init__(store, planner, rank)

    def plan_epoch(self) -> List[PlanBatch]:
        plan = super().plan_epoch()
        B = self.planner.batch_size
        draws = (torch.rand(len(plan) * B, 2, generator=self.gen) < 0.5).numpy()
        flips = (draws[:, 0] * FLIP_X + draws[:, 1] * FLIP_Y).astype(np.int32)
        return [pb._replace(flips=flips[i * B:(i + 1) * B]) for i, pb in enumerate(plan)]

    def gather(self, pb: PlanBatch) -> Batch:
        """The device batch of one plan entry (gather_beatmap_rows with the windows' flip masks)."""
        audio, chart, idx, _, _ = gather_beatmap_rows(self.store, self.pin, pb.maps, pb.starts, pb.lens, pb.Lpad, pb.flips, flip=True)
        return Batch(audio, chart, self.store.labels.index_select(0, idx))


class ResidentBeatmapValFeed:
    """Re-iterable over one validation epoch of the held-out maps in `store`, whole maps in ragged groups (`data.RaggedBeatmapBatch`).

    The plan is made once, from the store's lengths: a map of L frames pads to P = L rounded up to `pad_multiple` (the trainer's
    2 x chunk_size, what `LatentTrainer.pad_batch` pads a map to), and the maps are packed longest first (encode_latents.pack) into groups
    whose count x longest P stays within `frame_budget`; a map longer than the budget goes alone.  A group is gathered twice — whole maps
    (G, 72 | 9, Pmax), and their halves (2G, 72 | 9, Pmax / 2): row 2g frames [0, P_g / 2) of map g, row 2g + 1 frames [P_g / 2, L_g) —
    each time by three od_feed_gather_quant launches behind one descriptor copy, and od_replicate_tail then repeats every row's last frame
    up to its padded length.  The values are bit for bit those of read_spec / read_beatmap, .float() and pad_batch; there are no flips.

    A map shorter than `pad_multiple` frames pads to P = pad_multiple with a second half that may hold no frame of its own (nothing to
    replicate from inside that row), so such maps are not grouped: they follow the groups one by one as unpadded batch-1 `data.Batch`es,
    which `LatentTrainer.validation_step` pads and evaluates as it always has.  A spectrogram longer than its chart is cut to the chart's
    frames."""

    def __init__(self, store: ResidentBeatmapStore, pad_multiple: int, frame_budget: Optional[int] = None):
        from .encode_latents import DEFAULT_FRAME_BUDGET, pack
        if pad_multiple < 2 or pad_multiple % 2:
            raise ValueError(f"pad_multiple must be an even number of frames (2 x chunk_size), got {pad_multiple}")
        self.store, self.pad_multiple = store, int(pad_multiple)
        self.frame_budget = int(DEFAULT_FRAME_BUDGET if frame_budget is None else frame_budget)
        if self.frame_budget < 1:
            raise ValueError(f"data.val_frame_budget must be at least 1 frame, got {frame_budget}")
        self.plens = (store.lengths + self.pad_multiple - 1) // self.pad_multiple * self.pad_multiple
        whole = np.nonzero(store.lengths >= self.pad_multiple)[0]
        self.groups: List[np.ndarray] = [whole[g] for g in pack(self.plens[whole].tolist(), self.frame_budget)]
        self.short: np.ndarray = np.nonzero(store.lengths < self.pad_multiple)[0]
        self.pin = store.device.type == "cuda"

    def __len__(self):
        return len(self.groups) + len(self.short)

    def padded_share(self) -> List[float]:
        """Per group, the share of its G x Pmax frames that belong to no map (replicated tails and zeros)."""
        return [1.0 - float(self.store.lengths[g].sum()) / (len(g) * int(self.plens[g].max())) for g in self.groups]

    def _gather(self, maps: np.ndarray, starts: np.ndarray, lens: np.ndarray, plens: np.ndarray, Lpad: int):
        """(audio (B, 72, Lpad), chart (B, 9, Lpad), the maps' indices on the device): row i takes lens[i] frames of map maps[i] from
        starts[i], its last frame repeated up to plens[i], zeros behind; plens rides in the descriptor copy in the place of the flip masks."""
        assert (lens <= plens).all() and (plens <= Lpad).all()
        audio, chart, idx, lens32, plens32 = gather_beatmap_rows(self.store, self.pin, maps, starts, lens, Lpad, plens, flip=False)
        if (plens > lens).any():
            ops.replicate_tail(audio, lens32, plens32)
            ops.replicate_tail(chart, lens32, plens32)
        return audio, chart, idx

    def gather(self, maps: np.ndarray) -> RaggedBeatmapBatch:
        """The device batch of one group: its whole maps and their halves."""
        st = self.store
        L, P = st.lengths[maps], self.plens[maps]
        H = P // 2                                            # L > P - pad_multiple >= P / 2: both halves hold frames of the map
        audio, chart, idx = self._gather(maps, np.zeros_like(L), L, P, int(P.max()))
        two = np.repeat(maps, 2)
        starts, lens = np.stack([np.zeros_like(H), H], 1).reshape(-1), np.stack([H, L - H], 1).reshape(-1)
        audio_h, chart_h, _ = self._gather(two, starts, lens, np.repeat(H, 2), int(H.max()))
        return RaggedBeatmapBatch(audio, chart, st.labels.index_select(0, idx), torch.from_numpy(L.astype(np.int64)), audio_h, chart_h)

    def gather_one(self, m: int) -> Batch:
        """Map m alone and unpadded, as the host loader's batch-1 tuple."""
        maps = np.asarray([m], dtype=np.int64)
        L = self.store.lengths[maps]
        audio, chart, idx = self._gather(maps, np.zeros_like(L), L, L, int(L[0]))
        return Batch(audio, chart, self.store.labels.index_select(0, idx))

    def __iter__(self) -> Iterator:
        for g in self.groups:
            yield self.gather(g)
        for m in self.short.tolist():
            yield self.gather_one(m)


class ResidentBeatmapDataModule:
    """`BeatmapDataModule` with the training set resident on `device`: the same constructor keys (the YAML `data:` block of fit-latent)
    plus `device`, `resident_max_gb`, and `resident_val` with `val_frame_budget` and `val_pad_multiple`.  The host module holds out the
    validation mapsets and, unless `resident_val`, keeps the validation loader (whole maps read once per check), which is all
    `num_workers` still serves; `shuffle_buffer_size` serves nothing: an epoch is a full permutation of its windows.  With `resident_val`
    the held-out maps go, on first use, into a second store under the same `resident_max_gb`, and validation reads ragged groups from it
    (ResidentBeatmapValFeed); `val_pad_multiple` is the trainer's 2 x chunk_size (fit-latent passes it)."""

    def __init__(self, batch_size: int, seq_len: int, num_workers: int = 0, max_val_count: int = 512, max_val_frac: float = .3,
                 data_path: str = "./data", shuffle_buffer_size: int = 1, max_per_map: int = -1, rank: int = 0, world_size: int = 1,
                 device=None, resident_max_gb: Optional[float] = None, resident_val: bool = False, val_frame_budget: Optional[int] = None,
                 val_pad_multiple: Optional[int] = None):
        if seq_len is None:
            raise ValueError("data.resident trains fit-latent on fixed windows: data.seq_len must be an integer")
        if resident_val and val_pad_multiple is None:
            raise ValueError("data.resident_val pads every held-out map as the trainer does: val_pad_multiple (2 x the model's chunk_size) "
                             "is needed")
        self.host = BeatmapDataModule(batch_size, seq_len, num_workers, max_val_count, max_val_frac, data_path, shuffle_buffer_size, max_per_map,
                                      rank, world_size)
        self.device, self.rank = _device_or_default(device), rank
        max_bytes = _gb_to_bytes(resident_max_gb)
        self.store = ResidentBeatmapStore(self.host.train_set.mapsets, self.device, rank, world_size, max_bytes)
        self.planner = EpochPlanner(self.store.lengths, batch_size, int(seq_len), max_per_map)
        self.feed = ResidentBeatmapFeed(self.store, self.planner, rank)
        self.resident_val, self._max_bytes = bool(resident_val), max_bytes
        self._val_args = (val_pad_multiple, val_frame_budget)
        self.val_feed: Optional[ResidentBeatmapValFeed] = None

    def train_dataloader(self) -> ResidentBeatmapFeed:
        return self.feed

    def val_dataloader(self):
        if not self.resident_val:
            return self.host.val_dataloader()
        if self.val_feed is None:
            # refused, before anything is allocated, if it does not fit under resident_max_gb beside the training store
            val_store = ResidentBeatmapStore(self.host.val_set.mapsets, self.device, max_bytes=self._max_bytes, reserved_bytes=self.store.nbytes)
            self.val_feed = ResidentBeatmapValFeed(val_store, *self._val_args)
        return self.val_feed
