"""`encode-latents` — the latent model's encoding direction over a pre-processed dataset (reference:
osu_dreamer/scripts/encode_latents.py): for every `*.map.npy`, `<map>.latent.npz` {z (E, l), s (S,), labels}, and per mapset
directory `h.npy` (A, l) from its `spec.npy` — the files `fit-denoiser`'s feeder reads (data.py).

    python -m osu_dreamer_amd encode-latents --latent-ckpt-path latent.ckpt --data-dir ./data

Same outputs and skip rule as the reference: a map whose `.latent.npz` and `h.npy` both exist is skipped unless `--force`.  Where the
reference runs one map per call, maps and mapsets are packed into varlen calls of up to `--frame-budget` padded frames
(`LatentModel.encode_chart` / `audio_encoder` with `lengths=`), and the audio encoder runs once per mapset, not once per map.  The packing
reads only the arrays' headers; a call's files are read when that call runs and dropped after it, so host memory stays bounded by the
frame budget (or by the one longer map or song that goes alone), whatever the dataset's size.
"""
from __future__ import annotations

from dataclasses import asdict, is_dataclass
from pathlib import Path
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .data import beatmap_length, read_beatmap, read_spec, spec_length

PRECISIONS = {"fp32": (None, "f32"), "fp32_bf16x3": (None, "bf16x3"), "bf16": (torch.bfloat16, "f32")}
DEFAULT_FRAME_BUDGET = 1 << 19


def load_latent_ckpt(path: str, device="cuda"):
    """A latent-model fit checkpoint (`hyper_parameters` emb_dim, style_dim, n_downs, stride, latent_args; `latent.*` weights, the
    keys save_inference reads) -> LatentModel on `device`."""
    from .inference import dataclass_from_dict
    from .latent import LatentModel, LatentModelArgs
    ck = torch.load(path, map_location="cpu", weights_only=False)
    hp = ck["hyper_parameters"]
    la = hp["latent_args"]
    if is_dataclass(la) and not isinstance(la, type):
        la = asdict(la)
    model = LatentModel(hp["emb_dim"], hp["style_dim"], hp["n_downs"], hp["stride"], dataclass_from_dict(LatentModelArgs, dict(la)))
    sd = {k[len("latent."):]: v for k, v in ck["state_dict"].items() if k.startswith("latent.")}
    model.load_state_dict(sd)
    return model.to(device).eval()


def pack(lengths: Sequence[int], frame_budget: int) -> List[List[int]]:
    """Indices into `lengths`, longest first, in groups whose padded size (count x longest) stays within `frame_budget` (a single
    longer item goes alone)."""
    order = sorted(range(len(lengths)), key=lambda i: -lengths[i])
    groups: List[List[int]] = []
    for i in order:
        if groups and (len(groups[-1]) + 1) * lengths[groups[-1][0]] <= frame_budget:
            groups[-1].append(i)
        else:
            groups.append([i])
    return groups


def _stack(arrays: List[np.ndarray], c: int, dev) -> Tuple[torch.Tensor, List[int]]:
    """(C, L_i) float64 arrays -> (n, C, Lpad) fp32 on dev, each replicate-padded to a multiple of c (ldm.pad_to_multiple), then
    zero-padded to the longest; and the padded lengths."""
    from .ldm import pad_to_multiple
    padded = [pad_to_multiple(torch.from_numpy(a).float()[None], c)[0] for a in arrays]
    lens = [p.shape[-1] for p in padded]
    out = torch.zeros(len(padded), padded[0].shape[0], max(lens))
    for i, p in enumerate(padded):
        out[i, :, :lens[i]] = p
    return out.to(dev), lens


@torch.no_grad()
def encode_dataset(model, data_dir, force: bool = False, frame_budget: int = DEFAULT_FRAME_BUDGET,
                   progress: Optional[Callable[[str], None]] = None) -> Tuple[int, int]:
    """Encode every `*.map.npy` under `data_dir` with `model` (a LatentModel); returns (maps written, h.npy files written).  Files are read
    one packed call at a time."""
    data_dir = Path(data_dir)
    c, dev = model.chunk_size, next(model.parameters()).device
    map_files = sorted(data_dir.rglob("*.map.npy"))
    if len(map_files) == 0:
        raise RuntimeError(f"no pre-processed maps found in {data_dir}")
    todo, h_dirs, seen = [], [], set()
    for f in map_files:
        out_file = f.with_name(f.name[: -len(".map.npy")] + ".latent.npz")
        h_file = f.parent / "h.npy"
        if not force and out_file.exists() and h_file.exists():
            continue
        todo.append((f, out_file))
        if (force or not h_file.exists()) and f.parent not in seen:
            seen.add(f.parent)
            h_dirs.append(f.parent)

    # audio: once per mapset directory
    for grp in pack([-(-spec_length(d / "spec.npy") // c) * c for d in h_dirs], frame_budget):
        specs = [read_spec(h_dirs[i] / "spec.npy") for i in grp]
        audio, lens = _stack(specs, c, dev)
        del specs
        _, h = model.audio_encoder(audio, lengths=lens)
        h = h.float().cpu().numpy()
        for j, i in enumerate(grp):
            np.save(h_dirs[i] / "h.npy", np.ascontiguousarray(h[j, :, :lens[j] // c]))
            if progress:
                progress(str(h_dirs[i] / "h.npy"))
        del audio, h

    # charts
    for grp in pack([-(-beatmap_length(f) // c) * c for f, _ in todo], frame_budget):
        maps = [read_beatmap(todo[i][0]) for i in grp]
        chart, lens = _stack([mp[0] for mp in maps], c, dev)
        z, s = model.encode_chart(chart, lengths=lens)
        z, s = z.cpu().numpy(), s.cpu().numpy()
        for j, i in enumerate(grp):
            np.savez(todo[i][1], z=np.ascontiguousarray(z[j, :, :lens[j] // c]), s=s[j], labels=maps[j][1])
            if progress:
                progress(str(todo[i][1]))
        del maps, chart, z, s
    return len(todo), len(h_dirs)


def encode_latents(latent_ckpt_path: str = "latent.ckpt", data_dir: str = "./data", device: Optional[str] = None, force: bool = False,
                   precision: str = "fp32", frame_budget: int = DEFAULT_FRAME_BUDGET) -> Tuple[int, int]:
    """scripts/encode_latents.py on the HIP path: checkpoint + dataset directory -> cached encodings; returns (maps, h files) written."""
    from . import _lib
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
    if not Path(data_dir).is_dir():
        raise ValueError(f"data dir `{data_dir}` does not exist")
    _lib.lib()                                   # no CPU path: fail before loading anything else
    model = load_latent_ckpt(latent_ckpt_path, device=device or "cuda")
    model.compute_dtype, model.f32_matmul = PRECISIONS[precision]
    return encode_dataset(model, data_dir, force, frame_budget)


def add_parser(sub):
    p = sub.add_parser("encode-latents", help="precompute latent-model encodings (h, z, s, labels) for diffusion training")
    p.add_argument("--latent-ckpt-path", default="latent.ckpt", help="path to the latent checkpoint")
    p.add_argument("--data-dir", default="./data", help="pre-processed dataset directory")
    p.add_argument("--device", default=None, help="torch device (default: cuda)")
    p.add_argument("--force", action="store_true", help="overwrite existing cached latents")
    p.add_argument("--precision", default="fp32", choices=sorted(PRECISIONS))
    p.add_argument("--frame-budget", type=int, default=DEFAULT_FRAME_BUDGET,
                   help="padded frames per batched encoder call (songs / maps x the longest of them)")
    return p


def run(a):
    maps, hs = encode_latents(a.latent_ckpt_path, a.data_dir, a.device, a.force, a.precision, a.frame_budget)
    print(f"encoded {maps} maps and {hs} mapset audio files under {a.data_dir}")
