"""Feeder for the denoiser: cached latent encodings -> `LatentBatch`es.

Mirrors osu_dreamer/data/modules/latent.py:20-149 (on-disk format, window cropping, shuffle
buffer, mapset hold-out from data/modules/beatmap.py:33-71) so `encode-latents` output is read
unchanged.  MI355X-side differences: the stream is sharded by (rank, worker) — the reference
shards by worker only, so DDP ranks would see identical data — and there is no Lightning
dependency.  `write_synthetic_dataset` produces the same layout from seeded noise for
BASELINE configs[0] (no dataset ships with the repo).
"""
from __future__ import annotations

import random
from pathlib import Path
from typing import Iterator, List, NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch.utils.data import DataLoader, IterableDataset

NUM_LABELS = 5


def read_spec(path) -> np.ndarray:
    """A pre-processed `spec.npy` -> float64 (F, L): the stored unsigned integers scaled to [0, 1] by their dtype's maximum
    (data/load_audio.py:58-59)."""
    a = np.load(path)
    return a.astype(np.float64) / np.iinfo(a.dtype).max


def read_beatmap(path) -> Tuple[np.ndarray, np.ndarray]:
    """A pre-processed `<map>.map.npy` (an npz: hit, xy, xy_min, xy_rng, labels) -> (chart float64 (9, L), labels): the hit rows scaled
    to [0, 1], then the cursor rows mapped back to xy_min + [0, 1] * xy_rng, each scale taken from the array's integer dtype
    (data/beatmap/encode.py:81-87)."""
    with np.load(path) as d:
        hit, xy, xy_min, xy_rng, labels = d["hit"], d["xy"], d["xy_min"], d["xy_rng"], d["labels"]
    chart = np.concatenate([hit.astype(np.float64) / np.iinfo(hit.dtype).max,
                            xy.astype(np.float64) / np.iinfo(xy.dtype).max * xy_rng + xy_min])
    return chart, labels


def spec_length(path) -> int:
    """Frames of a `spec.npy`, from its header (the array is not read)."""
    return int(np.load(path, mmap_mode="r").shape[-1])


def beatmap_length(path) -> int:
    """Frames of a `<map>.map.npy`, from the header of its `hit` member (the arrays are not read)."""
    import zipfile
    with zipfile.ZipFile(path) as z, z.open("hit.npy") as f:
        version = np.lib.format.read_magic(f)
        read = np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0
        shape, _, _ = read(f)
    return int(shape[-1])


class LatentBatch(NamedTuple):
    h: torch.Tensor        # (A, l) audio features at latent rate
    z: torch.Tensor        # (E, l) chart latent
    s: torch.Tensor        # (S,)   per-map style code
    labels: torch.Tensor   # (NUM_LABELS,)


class RaggedLatentBatch(NamedTuple):
    """N whole maps of different lengths, zero-padded to a common Lpad: map b is valid for frames < lengths[b].  What
    `LatentDataModule(seq_len=None, batch_size=N > 1)` collates (and, with `batch_frames`, what its bucketed loader yields, N = 1 included)
    and `DiffusionTrainer.training_step` accepts beside the 4-tuple."""
    h: torch.Tensor        # (N, A, Lpad)
    z: torch.Tensor        # (N, E, Lpad)
    s: torch.Tensor        # (N, S)
    labels: torch.Tensor   # (N, NUM_LABELS)
    lengths: torch.Tensor  # (N,) int64, on the host


class RaggedLatentValBatch(NamedTuple):
    """G whole held-out maps for the denoiser's validation (resident.ResidentLatentValFeed), each already cut into the val_batches
    segments `DiffusionTrainer.validation_step` cuts a map into: with seg_g = L_g // val_batches, row offs[g] + j is frames
    [j * seg_g, (j + 1) * seg_g) of map g's z and of its mapset's h, zeros behind seg_g up to Lpad; every row of map g has length seg_g
    (>= 1).  R = G * val_batches rows.  What `DiffusionTrainer.validation_step` accepts beside the batch-1 tuple."""
    h: torch.Tensor        # (R, A, Lpad)
    z: torch.Tensor        # (R, E, Lpad)
    s: torch.Tensor        # (G, S)
    labels: torch.Tensor   # (G, NUM_LABELS)
    lengths: torch.Tensor  # (R,) int64, on the host
    offs: torch.Tensor     # (G + 1,) int64, on the host: map g's rows are [offs[g], offs[g + 1])


class RaggedBeatmapBatch(NamedTuple):
    """G whole held-out maps of different lengths for the latent model's validation (resident.ResidentBeatmapValFeed), padded as
    `LatentTrainer.pad_batch` pads each of them alone: map g has lengths[g] frames, then its last frame repeated up to
    P_g = lengths[g] rounded up to the feed's pad multiple (2 x chunk_size), then zeros up to Pmax = the longest P_g.  The same maps cut in
    halves come with them, as `latent_train.split_halves` cuts a padded map: row 2g is frames [0, P_g / 2) of map g, row 2g + 1 is frames
    [P_g / 2, P_g), zeros behind.  What `LatentTrainer.validation_step` accepts beside the batch-1 tuple."""
    audio: torch.Tensor          # (G, A_DIM, Pmax)
    chart: torch.Tensor          # (G, X_DIM, Pmax)
    labels: torch.Tensor         # (G, NUM_LABELS)
    lengths: torch.Tensor        # (G,) int64, on the host: the maps' own frames, before any padding
    audio_halves: torch.Tensor   # (2G, A_DIM, Pmax / 2)
    chart_halves: torch.Tensor   # (2G, X_DIM, Pmax / 2)


def collate_ragged(samples: List[LatentBatch], pad_multiple: int = 64) -> RaggedLatentBatch:
    """Whole maps -> one RaggedLatentBatch, zero-padded to the longest map rounded up to `pad_multiple` (few distinct padded lengths: the
    engine keeps one workspace per (N, Lpad))."""
    lens = [int(b.z.size(-1)) for b in samples]
    Lpad = (max(lens) + pad_multiple - 1) // pad_multiple * pad_multiple
    h = torch.zeros(len(samples), samples[0].h.size(0), Lpad)
    z = torch.zeros(len(samples), samples[0].z.size(0), Lpad)
    for i, (b, n) in enumerate(zip(samples, lens)):
        h[i, :, :n], z[i, :, :n] = b.h[..., :n], b.z
    return RaggedLatentBatch(h, z, torch.stack([b.s for b in samples]), torch.stack([b.labels for b in samples]),
                             torch.tensor(lens, dtype=torch.int64))


def _roundup(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def cut_batches(lengths: List[int], batch_frames: int, batch_size: int, pad_multiple: int = 64) -> List[List[int]]:
    """Indices of `lengths` grouped into frame-budget batches: sorted by length (longest first, ties in arrival order) and cut greedily — a
    batch opened by a map of n frames has Lpad = roundup(n, pad_multiple) and takes the next-shorter maps while (count + 1) * Lpad <=
    batch_frames and count < batch_size.  Every index appears once; a map whose Lpad alone exceeds the budget still gets a batch of its own
    (LatentDataModule refuses the configuration that could produce one)."""
    order = sorted(range(len(lengths)), key=lambda i: -lengths[i])          # sorted() is stable: ties keep arrival order
    out: List[List[int]] = []
    i = 0
    while i < len(order):
        Lpad = _roundup(lengths[order[i]], pad_multiple)
        n = 1
        while i + n < len(order) and n < batch_size and (n + 1) * Lpad <= batch_frames:
            n += 1
        out.append(order[i:i + n])
        i += n
    return out


class BucketedBatches(IterableDataset):
    """Length-bucketed, frame-budget batches over a whole-map LatentDataset, per loader worker: gather `bucket_pool` samples of the dataset's
    stream (after its shard, shuffle buffer and max_len window), cut them with `cut_batches`, shuffle the pool's batches with the worker's
    RNG (the `random` module, seeded by LatentDataset.__iter__: a run is reproducible from its seed) and yield each as a RaggedLatentBatch.
    The partial pool at the end of the stream is cut the same way: no map is dropped."""

    def __init__(self, dataset: "LatentDataset", batch_frames: int, batch_size: int, bucket_pool: int, pad_multiple: int = 64):
        super().__init__()
        self.dataset, self.batch_frames, self.batch_size = dataset, batch_frames, batch_size
        self.bucket_pool, self.pad_multiple = bucket_pool, pad_multiple

    def _cut(self, pool: List[LatentBatch]) -> Iterator[RaggedLatentBatch]:
        groups = cut_batches([int(b.z.size(-1)) for b in pool], self.batch_frames, self.batch_size, self.pad_multiple)
        random.shuffle(groups)
        for g in groups:
            yield collate_ragged([pool[i] for i in g], self.pad_multiple)

    def __iter__(self):
        pool: List[LatentBatch] = []
        for sample in self.dataset:
            pool.append(sample)
            if len(pool) == self.bucket_pool:
                yield from self._cut(pool)
                pool = []
        if pool:
            yield from self._cut(pool)


def load_latents(latent_file: Path) -> LatentBatch:
    """`<map>.latent.npz` {z, s, labels} + sibling `h.npy` (latent.py:74-80)."""
    with np.load(latent_file) as d:
        z, s, labels = (torch.from_numpy(d[k]).float() for k in ("z", "s", "labels"))
    h = torch.from_numpy(np.load(latent_file.parent / "h.npy")).float()
    return LatentBatch(h, z, s, labels)


def split_mapsets(mapsets: List[Path], counts: List[int], max_val_count: int, max_val_frac: float) -> Tuple[List[Path], List[Path]]:
    """The hold-out rule of data/modules/beatmap.py:38-71 on an ORDERED list of mapsets with their map counts: walk the
    list, a mapset goes to validation while the validation set stays within min(max_val_count, int(total * max_val_frac))
    maps, otherwise to training."""
    full = sum(counts)
    if full == 0:
        raise ValueError("data dir is empty, generate dataset first")
    if max_val_count <= 0:
        raise ValueError(f"invalid {max_val_count=}")
    if not (0 < max_val_frac < 1):
        raise ValueError(f"invalid {max_val_frac=}")
    cap = min(max_val_count, int(full * max_val_frac))
    if not (0 < cap < full):
        raise ValueError(f"invalid max_val_size={cap} given full_size={full} {max_val_count=} {max_val_frac=}")
    train, val, nval = [], [], 0
    for mapset, n in zip(mapsets, counts):
        if nval + n > cap:
            train.append(mapset)
        else:
            val.append(mapset)
            nval += n
    return train, val


def hold_out_mapsets(data_dir: Path, pattern: str, max_val_count: int, max_val_frac: float) -> Tuple[List[Path], List[Path]]:
    """Whole mapsets (directories) are held out so train/val never share audio.  The reference walks
    `data_dir.iterdir()` in file-system order, so its split differs from machine to machine; here the listing is sorted,
    which every rank of a data-parallel run needs anyway (all ranks must hold out the SAME mapsets)."""
    if not data_dir.exists():
        raise ValueError(f"data dir `{data_dir}` does not exist, generate dataset first")
    mapsets = sorted(data_dir.iterdir())
    counts = [sum(1 for _ in m.glob(pattern)) for m in mapsets] if mapsets else []
    extra = sum(1 for _ in data_dir.rglob(pattern)) - sum(counts)      # maps nested deeper count towards the total (rglob)
    if sum(counts) + extra == 0:
        raise ValueError(f"data dir `{data_dir}` is empty, generate dataset first")
    if extra:
        mapsets, counts = mapsets + [None], counts + [extra]
    train, val = split_mapsets(mapsets, counts, max_val_count, max_val_frac)
    return [m for m in train if m is not None], [m for m in val if m is not None]


class LatentDataset(IterableDataset):
    def __init__(self, mapsets: List[Path], seq_len: Optional[int] = None, shuffle_buffer_size: int = 1,
                 max_per_map: int = -1, rank: int = 0, world_size: int = 1, max_len: Optional[int] = None):
        """`max_len` (whole maps, seq_len None, only): a map longer than that contributes one random window of max_len frames."""
        super().__init__()
        self.mapsets, self.seq_len, self.max_len = mapsets, seq_len, max_len
        self.shuffle_buffer_size = shuffle_buffer_size
        self.max_per_map = max_per_map if max_per_map > 0 else float("inf")
        self.rank, self.world_size = rank, world_size

    def _files(self) -> Iterator[Path]:
        return (f for m in self.mapsets for f in sorted(m.glob("*.latent.npz")))

    def _stream(self, nshards: int, shard: int) -> Iterator[LatentBatch]:
        for i, f in enumerate(self._files()):
            if i % nshards == shard:
                yield from self.make_samples(f)

    def __iter__(self):
        info = torch.utils.data.get_worker_info()
        nw, wid, seed = (1, 0, torch.initial_seed()) if info is None else (info.num_workers, info.id, info.seed)
        random.seed(seed + 7919 * self.rank)
        stream = self._stream(nw * self.world_size, self.rank * nw + wid)
        if self.shuffle_buffer_size <= 1:
            yield from stream
            return
        buf: List[LatentBatch] = []
        for sample in stream:
            if len(buf) < self.shuffle_buffer_size:
                buf.append(sample)
                continue
            j = random.randrange(len(buf))
            yield buf[j]
            buf[j] = sample
        random.shuffle(buf)
        yield from buf

    def make_samples(self, latent_file: Path) -> Iterator[LatentBatch]:
        h, z, s, labels = load_latents(latent_file)
        if self.seq_len is None:
            L = z.size(-1)
            if self.max_len is not None and L > self.max_len:
                i = int(torch.randint(0, L - self.max_len + 1, ()).item())
                h, z = h[..., i:i + self.max_len].clone(), z[..., i:i + self.max_len].clone()
            yield LatentBatch(h, z, s, labels)
            return
        end = z.size(-1) - self.seq_len + 1
        if end < 1:
            return
        start = int(torch.randint(0, min(self.seq_len, end), ()).item())
        idxs = torch.arange(start, end, self.seq_len)
        idxs = idxs[torch.randperm(len(idxs))[: int(min(self.max_per_map, len(idxs)))]]
        for i in idxs:
            yield LatentBatch(h[..., i:i + self.seq_len].clone(), z[..., i:i + self.seq_len].clone(), s, labels)


class LatentDataModule:
    """Same constructor keys as the reference's LatentDataModule (they are the YAML `data:` block), plus `max_len` and `pad_multiple` for
    ragged training: with `seq_len: null` and `batch_size` N > 1 the training loader collates N whole maps into one `RaggedLatentBatch`,
    zero-padded to the longest map rounded up to `pad_multiple`; a map longer than `max_len` contributes a random window of `max_len`
    frames, which bounds the step's memory.  With an integer `seq_len` nothing changes.

    `batch_frames` F (with `seq_len: null` and `max_len` only) sizes a batch by its padded frames instead of its songs: every batch holds
    B * Lpad <= F, `batch_size` becomes the cap on B, and maps of similar length share a batch (BucketedBatches: each worker sorts a pool of
    `bucket_pool` maps by length and cuts it from the longest).  No map is dropped.  `bucket_pool` defaults to 64 x `batch_size`: a pool holds
    whole maps on the host, per worker (0.8 MB for 1500 latent frames at the default widths, so 0.4 GB at batch_size 8), and the padding
    left in a batch falls with the number of maps that are sorted together, so the default gathers 64 full batches' worth before it cuts.
    Without `batch_frames` the loaders are what they were."""

    def __init__(self, batch_size: int, seq_len: Optional[int], num_workers: int, max_val_count: int = 512,
                 max_val_frac: float = .3, data_path: str = "./data", shuffle_buffer_size: int = 1,
                 max_per_map: int = -1, rank: int = 0, world_size: int = 1, max_len: Optional[int] = None, pad_multiple: int = 64,
                 batch_frames: Optional[int] = None, bucket_pool: Optional[int] = None):
        self.batch_size, self.seq_len, self.num_workers = batch_size, seq_len, num_workers
        if seq_len is not None and max_len is not None:
            raise ValueError("data.max_len bounds whole maps: it applies with seq_len: null only")
        if max_len is not None and max_len < 1 or pad_multiple < 1:
            raise ValueError(f"invalid {max_len=} / {pad_multiple=}")
        self.max_len, self.pad_multiple = max_len, int(pad_multiple)
        if batch_frames is None and bucket_pool is not None:
            raise ValueError("data.bucket_pool is the pool of the frame-budget loader: set data.batch_frames, or drop data.bucket_pool")
        if batch_frames is not None:
            if seq_len is not None:
                raise ValueError("data.batch_frames sizes batches of whole maps: set data.seq_len: null, or drop data.batch_frames")
            if max_len is None:
                raise ValueError("data.batch_frames needs data.max_len: without it one long map could exceed the frame budget")
            if batch_size < 1:
                raise ValueError(f"data.batch_size is the cap on songs per batch under data.batch_frames: it must be >= 1, got {batch_size}")
            if _roundup(int(max_len), self.pad_multiple) > int(batch_frames):
                raise ValueError(f"data.max_len={max_len} rounded up to data.pad_multiple={pad_multiple} is {_roundup(int(max_len), self.pad_multiple)} "
                                 f"frames, more than data.batch_frames={batch_frames}: raise data.batch_frames or lower data.max_len")
            bucket_pool = 64 * batch_size if bucket_pool is None else int(bucket_pool)
            if bucket_pool < 1:
                raise ValueError(f"data.bucket_pool must be >= 1, got {bucket_pool}")
        self.batch_frames = None if batch_frames is None else int(batch_frames)
        self.bucket_pool = bucket_pool
        self.ragged = seq_len is None and (batch_size > 1 or batch_frames is not None)
        train, val = hold_out_mapsets(Path(data_path), "*.latent.npz", max_val_count, max_val_frac)
        self.train_set = LatentDataset(train, seq_len, shuffle_buffer_size, max_per_map, rank, world_size, max_len=max_len)
        self.val_set = LatentDataset(val)

    def train_dataloader(self):
        if self.batch_frames is not None:             # the dataset yields ready RaggedLatentBatches
            return DataLoader(BucketedBatches(self.train_set, self.batch_frames, self.batch_size, self.bucket_pool, self.pad_multiple),
                              batch_size=None, num_workers=self.num_workers, pin_memory=True, persistent_workers=self.num_workers > 0)
        collate = {"collate_fn": self._collate} if self.ragged else {}
        return DataLoader(self.train_set, batch_size=self.batch_size, num_workers=self.num_workers, pin_memory=True,
                          persistent_workers=self.num_workers > 0, drop_last=True, **collate)

    def _collate(self, samples):
        return collate_ragged(samples, self.pad_multiple)

    def val_dataloader(self):
        return DataLoader(self.val_set, batch_size=1, num_workers=min(1, self.num_workers), pin_memory=True,
                          persistent_workers=self.num_workers > 0)


def write_synthetic_dataset(data_path: str, n_maps: int = 8, frames=4096, a_dim: int = 128, emb_dim: int = 6,
                            style_dim: int = 32, seed: int = 0):
    """`n_maps` mapset dirs each with h.npy (A, frames) and 0.latent.npz {z (E, frames), s (S,), labels (5,)}:
    h ~ N(0,1), z per-frame RMS-normalised, s RMS-normalised.  `frames` may be a list (one length per map)."""
    rng = np.random.default_rng(seed)
    root = Path(data_path)
    lengths = list(frames) if isinstance(frames, (list, tuple)) else [frames] * n_maps
    for i in range(n_maps):
        d = root / f"{i:04d}"
        d.mkdir(parents=True, exist_ok=True)
        frames = lengths[i]
        z = rng.standard_normal((emb_dim, frames)).astype(np.float32)
        z /= np.sqrt((z * z).mean(0, keepdims=True) + 1e-6)
        s = rng.standard_normal(style_dim).astype(np.float32)
        s /= np.sqrt((s * s).mean() + 1e-6)
        np.save(d / "h.npy", rng.standard_normal((a_dim, frames)).astype(np.float32))
        np.savez(d / "0.latent.npz", z=z, s=s, labels=(rng.random(NUM_LABELS) * 10).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- latent-model feeder
A_DIM, X_DIM = 72, 9
CURSOR_X, CURSOR_Y = 7, 8              # data/beatmap/encode.py: BeatmapEncoding.X, .Y


class Batch(NamedTuple):
    audio: torch.Tensor    # (A_DIM, L) spectrogram
    chart: torch.Tensor    # (X_DIM, L) encoded beatmap
    labels: torch.Tensor   # (NUM_LABELS,)


class BeatmapDataset(IterableDataset):
    """`<mapset>/spec.npy` + `<mapset>/<map>.map.npy` -> `Batch`es (data/modules/beatmap.py:119-207).  seq_len None: whole maps (validation);
    otherwise `seq_len` windows from a random start offset, at most `max_per_map` of them per map in random order, each with the x / y flip
    augmentation (v <- 1 - v on a cursor channel, with probability 1/2 each).  Files are sharded by (rank, worker), as LatentDataset's."""

    def __init__(self, mapsets: List[Path], seq_len: Optional[int] = None, shuffle_buffer_size: int = 1, max_per_map: int = -1,
                 rank: int = 0, world_size: int = 1):
        super().__init__()
        self.mapsets, self.seq_len = mapsets, seq_len
        self.shuffle_buffer_size = shuffle_buffer_size
        self.max_per_map = max_per_map if max_per_map > 0 else float("inf")
        self.rank, self.world_size = rank, world_size

    def _files(self) -> Iterator[Path]:
        return (f for m in self.mapsets for f in sorted(m.glob("*.map.npy")))

    def _stream(self, nshards: int, shard: int) -> Iterator[Batch]:
        for i, f in enumerate(self._files()):
            if i % nshards == shard:
                yield from self.make_samples(f)

    __iter__ = LatentDataset.__iter__          # seeding, (rank, worker) shard and shuffle buffer are the latent feeder's

    def make_samples(self, map_file: Path) -> Iterator[Batch]:
        audio = torch.from_numpy(read_spec(map_file.parent / "spec.npy")).float()
        chart_arr, label_arr = read_beatmap(map_file)
        chart, labels = torch.from_numpy(chart_arr).float(), torch.from_numpy(np.asarray(label_arr)).float()
        if self.seq_len is None:
            yield Batch(audio, chart, labels)
            return
        end = chart.size(-1) - self.seq_len + 1
        if end < 1:
            return
        start = int(torch.randint(0, min(self.seq_len, end), ()).item())
        idxs = torch.arange(start, end, self.seq_len)
        idxs = idxs[torch.randperm(len(idxs))[: int(min(self.max_per_map, len(idxs)))]]
        for i in idxs:
            window = chart[..., i:i + self.seq_len].clone()
            if torch.rand(()) < 0.5:
                window[CURSOR_X].mul_(-1).add_(1)
            if torch.rand(()) < 0.5:
                window[CURSOR_Y].mul_(-1).add_(1)
            yield Batch(audio[..., i:i + self.seq_len].clone(), window, labels)       # cloned: the buffer must not pin the whole spectrogram


class BeatmapDataModule:
    """Same constructor keys as the reference's BeatmapDataModule (the YAML `data:` block of fit-latent)."""

    def __init__(self, batch_size: int, seq_len: int, num_workers: int, max_val_count: int = 512, max_val_frac: float = .3,
                 data_path: str = "./data", shuffle_buffer_size: int = 1, max_per_map: int = -1, rank: int = 0, world_size: int = 1):
        self.batch_size, self.seq_len, self.num_workers = batch_size, seq_len, num_workers
        train, val = hold_out_mapsets(Path(data_path), "*.map.npy", max_val_count, max_val_frac)
        self.train_set = BeatmapDataset(train, seq_len, shuffle_buffer_size, max_per_map, rank, world_size)
        self.val_set = BeatmapDataset(val)

    def train_dataloader(self):
        return DataLoader(self.train_set, batch_size=self.batch_size, num_workers=self.num_workers, pin_memory=True,
                          persistent_workers=self.num_workers > 0, drop_last=True)

    def val_dataloader(self):
        return DataLoader(self.val_set, batch_size=1, num_workers=min(1, self.num_workers), pin_memory=True,
                          persistent_workers=self.num_workers > 0)


def write_synthetic_beatmaps(data_path: str, n_mapsets: int = 8, maps_per_set: int = 2, frames=4096, seed: int = 0):
    """`n_mapsets` mapset dirs each with spec.npy (uint8 (A_DIM, frames)) and `maps_per_set` files `<n>.map.npy` in the format read_beatmap
    reads (an npz: hit uint8 (7, L), xy uint16 (2, L), xy_min, xy_rng, labels), from seeded noise.  `frames` may be a list (one length
    per mapset)."""
    rng = np.random.default_rng(seed)
    root = Path(data_path)
    lengths = list(frames) if isinstance(frames, (list, tuple)) else [frames] * n_mapsets
    for i in range(n_mapsets):
        d = root / f"{i:04d}"
        d.mkdir(parents=True, exist_ok=True)
        L = lengths[i]
        np.save(d / "spec.npy", rng.integers(0, 256, (A_DIM, L), dtype=np.uint8))
        for n in range(maps_per_set):
            hit = rng.random((X_DIM - 2, L))
            hit[rng.random(hit.shape) < 0.5] = 0.0
            xy = np.cumsum(rng.standard_normal((2, L)) * 8, axis=1) + np.array([[256.], [192.]])
            xy_min = xy.min(axis=1, keepdims=True)
            xy_rng = xy.max(axis=1, keepdims=True) - xy_min
            xy_rng[xy_rng == 0.] = 1.
            with open(d / f"{n}.map.npy", "wb") as f:
                np.savez(f, hit=np.round(hit * 255).astype(np.uint8), xy=np.round((xy - xy_min) / xy_rng * 65535).astype(np.uint16),
                         xy_min=xy_min, xy_rng=xy_rng, labels=rng.random(NUM_LABELS) * 10)
