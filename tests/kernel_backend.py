"""Shared plumbing for kernel tests: the same test bodies run against
  * the SIMT-emulator build of the kernel sources (CPU, `-m "not gpu"`), and
  * the real gfx950 library on an MI355X (`-m gpu`).
"""
import math
import os
import subprocess

import pytest
import torch

from osu_dreamer_amd import _lib, det

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libod_emu.so")


_built = False


def build_emu():
    """Build (once per process, one process at a time: pytest-xdist workers share the tree) the emulator library."""
    global _built
    if not _built:
        import fcntl
        with open(os.path.join(EMU_DIR, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.check_call(["bash", os.path.join(EMU_DIR, "build_emu.sh")], stdout=subprocess.DEVNULL)
        _built = True
    return EMU_SO


BACKENDS = [
    pytest.param("emu", id="emu"),
    pytest.param("hip", id="hip", marks=pytest.mark.gpu),
]


@pytest.fixture(params=BACKENDS)
def dev(request):
    """Binds the library for the backend and returns the torch device to allocate on."""
    if request.param == "emu":
        if not _built or _lib.loaded_path() != EMU_SO:       # bound already: binding parses the header again, ~10 ms a test
            _lib.use_library(build_emu())
        return torch.device("cpu")
    if not torch.cuda.is_available():
        pytest.skip("hip backend selected but no GPU is visible")
    _lib._lib = None          # force the real library (raises if it was not built)
    _lib.lib()
    return torch.device("cuda:0")


def frames(x):   # (B,C,L) -> [B*L, C]
    B, C, L = x.shape
    return x.permute(0, 2, 1).reshape(B * L, C).contiguous()


def unframes(x, B, L):   # [B*L, C] -> (B,C,L)
    return x.reshape(B, L, -1).permute(0, 2, 1).contiguous()


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def block_errors(a, b, rows=64, floor=1e-3, scale=None, floor_max=1e-5):
    """Relative L2 error per block of `rows` rows, and over everything.  a, b: (..., L, C) — e.g. (batch, head, L, head_dim); the last
    block of each leading index may be ragged.  A block's denominator is at least `floor` x the median block norm of b and `floor_max` x
    the largest, so blocks whose reference cancels to about zero (or carries no weight at all) do not dominate.  `scale` (same shape as b):
    measure against its norms instead of b's — the magnitude a sum's rounding is relative to when its terms cancel.
    Returns (per-block errors of shape (..., blocks), global error)."""
    a, b = a.detach().double(), b.detach().double()
    L = a.shape[-2]
    nb = (L + rows - 1) // rows
    pad = nb * rows - L
    d = torch.nn.functional.pad((a - b).pow(2).sum(-1), (0, pad))
    r = torch.nn.functional.pad((b if scale is None else scale.double()).pow(2).sum(-1), (0, pad))
    err = d.reshape(*d.shape[:-1], nb, rows).sum(-1).sqrt()
    ref = r.reshape(*r.shape[:-1], nb, rows).sum(-1).sqrt()
    den = ref.clamp_min(max(floor * float(ref.flatten().median()), floor_max * float(ref.max())) + 1e-300)
    return err / den, float(d.sum().sqrt() / (r.sum().sqrt() + 1e-300))


def block_rel_l2(a, b, rows=64, floor=1e-3, scale=None, floor_max=1e-5):
    """block_errors reduced: (max block error, global error, index of the worst block).  NaN anywhere counts as the worst."""
    blk, glob = block_errors(a, b, rows, floor, scale, floor_max)
    flat = blk.flatten()
    worst = int(torch.nan_to_num(flat, nan=float("inf")).argmax())
    return float(flat[worst]), glob, tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), blk.shape))


def tile_errors(a, b, tr, tc, floor=1e-3, scale=None, floor_max=1e-5):
    """block_errors over 2-D output tiles: relative L2 per (tr x tc) tile of the matrices a, b (M, N) — the last tile row / column may be
    ragged — and over everything, with the same denominator floors and `scale` as block_errors.
    Returns (per-tile errors of shape (ceil(M / tr), ceil(N / tc)), global error)."""
    a, b = a.detach().double(), b.detach().double()
    M, N = a.shape
    tm, tn = (M + tr - 1) // tr, (N + tc - 1) // tc
    pad = (0, tn * tc - N, 0, tm * tr - M)
    d = torch.nn.functional.pad((a - b).pow(2), pad)
    r = torch.nn.functional.pad((b if scale is None else scale.double()).pow(2), pad)
    err = d.reshape(tm, tr, tn, tc).sum((1, 3)).sqrt()
    ref = r.reshape(tm, tr, tn, tc).sum((1, 3)).sqrt()
    den = ref.clamp_min(max(floor * float(ref.flatten().median()), floor_max * float(ref.max())) + 1e-300)
    return err / den, float(d.sum().sqrt() / (r.sum().sqrt() + 1e-300))


def tile_rel_l2(a, b, tr, tc, floor=1e-3, scale=None, floor_max=1e-5):
    """tile_errors reduced: (max tile error, global error, (tile row, tile column) of the worst tile).  NaN anywhere counts as the worst."""
    blk, glob = tile_errors(a, b, tr, tc, floor, scale, floor_max)
    flat = blk.flatten()
    worst = int(torch.nan_to_num(flat, nan=float("inf")).argmax())
    return float(flat[worst]), glob, (worst // blk.shape[1], worst % blk.shape[1])


TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2}


NAN = float("nan")


# ---------------------------------------------------------------- fenced buffers
class Fenced:
    """A (rows, cols) view at column 8 of a NaN buffer with >= 24 NaN columns behind it (ld a multiple of 8) and 3 NaN rows below."""

    def __init__(self, rows, cols, dtype, device, fill=None):
        self.rows, self.cols = rows, cols
        self.buf = torch.full((rows + 3, (cols + 32 + 7) // 8 * 8), NAN, dtype=dtype, device=device)
        self.v = self.buf[:rows, 8:8 + cols]
        if fill is not None:
            self.v.copy_(fill)

    def check(self, case, what):
        nan = torch.isnan(self.buf.float())
        inside = torch.zeros_like(nan)
        inside[:self.rows, 8:8 + self.cols] = True
        out = int((~nan & ~inside).sum())
        assert out == 0, f"{case}: {out} elements outside {what}[{self.rows}, {self.cols}] were written"
        bad = nan[:self.rows, 8:8 + self.cols]
        if bool(bad.any()):
            r, c = (int(i) for i in bad.nonzero()[0])
            raise AssertionError(f"{case}: {int(bad.sum())} elements of {what} are NaN (unwritten, or read from the poisoned padding), "
                                 f"first (frame {r}, column {c})")


class Flat:
    """A contiguous tensor of `shape` with 64 NaN elements either side (fp32 vectors: inv_rms, ssg, the weight gradients)."""

    def __init__(self, shape, device, fill=None, dtype=torch.float32):
        n = math.prod(shape)
        self.n = n
        self.buf = torch.full((n + 128,), NAN, dtype=dtype, device=device)
        self.v = self.buf[64:64 + n].view(*shape)
        if fill is not None:
            self.v.copy_(fill)

    def check(self, case, what):
        assert bool(torch.isnan(self.buf[:64]).all() & torch.isnan(self.buf[64 + self.n:]).all()), f"{case}: written outside {what}"
        bad = torch.isnan(self.v)
        assert not bool(bad.any()), f"{case}: {int(bad.sum())} elements of {what} are NaN, first {tuple(int(i) for i in bad.nonzero()[0])}"


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def det_run(device, on, outs, fn):
    """fn() with the deterministic shadow on (outs registered, flushed afterwards) or off."""
    if not on:
        fn()
        return
    try:
        det.force(True)
        ctx = det.context(device)
        for t in outs:
            ctx.register(t)
        fn()
        for t in outs:
            ctx.flush(t)
    finally:
        det.force(None)
