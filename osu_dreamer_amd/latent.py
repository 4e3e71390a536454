"""`LatentModel` on the HIP path: inference — the steps either side of `diffusion.sample` in `LDM.sample`
(osu_dreamer/models/inference/model.py:48,51; reference model: osu_dreamer/models/latent/model.py:38-134,
unet.py:21-126, spec_features.py:10-32).

Same constructor, same `state_dict()` keys and shapes as the reference's `LatentModel` (all of them, so a
reference checkpoint / inference artifact loads with `strict=True`), and the calls `LDM.sample` makes:

    skips, h = model.audio_encoder(audio)           # (Ba,72,L) -> [ (Ba,h_dim,L/stride^i) ], (Ba,h_dim,L/stride^n)
    chart, labels = model.decode(z, s, skips=skips) # or audio=...;   also decode_logits(z, s, ...)
    z, s = model.encode_chart(chart)                # (B,9,L) -> (B,emb_dim,L/chunk), (B,style_dim)

Each call also takes sequences of different lengths at once (`lengths=`, no-grad, the varlen kernels): they are stacked zero-padded to
a common length, each keeps to its own frames, and every frame past a sequence's length comes back as exactly 0:

    skips, h = model.audio_encoder(audio, lengths=Ls)                   # audio (G,72,Lpad), Ls[g] a multiple of chunk_size
    chart, labels = model.decode(z, s, skips=skips, lengths=Ls, offs=offs)  # z (B,E,Lpad/chunk): rows offs[g]:offs[g+1] are song g's
    z, s = model.encode_chart(chart, lengths=Ls)                        # chart (B,9,Lpad), one length per map

Activations are frame-major [B*L][h_dim] on the device; the tensors handed back are (B, C, L)-shaped *views* of
those buffers (no transposing copy), and `decode` takes them back without one.  `encode_chart(chart) -> (z, s)`
(chart encoder, style head, temporal head: the dataset-encoding direction of scripts/encode_latents.py) runs on
the same kernels.

Gradients (latent_grad.py).  Parameters are created with requires_grad = False, and with grad disabled or nothing requiring grad every
call above takes the no-grad path, bit for bit as before.  After `model.requires_grad_(True)` (or when a `z`, `s` or skip input requires
grad) `audio_encoder`, `encode_chart`, `decode_logits` and `forward` run as autograd Functions over the backward kernels of
csrc/latent.hip: every parameter's `.grad` is filled, and gradients flow to `z` and `s` of `decode_logits` / `forward`, to the skips
and `h` of `audio_encoder` (summed over the decoder rows when one audio row serves them all) and through the `z` and `s` that
`encode_chart` returns, so the body of the reference's `LatentTrainer.forward` and any torch optimizer run on top of this model.  fp32 and
`compute_dtype = torch.bfloat16` (bf16 activations and GEMM operands, fp32 accumulation and parameter gradients; the SpecFeatures front
end up to its SiLU stays fp32 on the grad path, so in bf16 the training forward is not bit for bit the no-grad forward of the same
model: the two differ by the bf16 rounding of that front end); `lengths=` and `f32_matmul = "bf16x3"` raise NotImplementedError with grad; `decode` stays no-grad.  Packed GEMM operands follow the parameters'
version counters, so an optimizer's in-place step needs no `invalidate()`.  A graph is backpropagated once: a second backward through the
same forward (retain_graph) raises, because the parameter gradients of a call are sums the kernels add into.

One forward.  The launch sequence of the layer, the two encoders, both heads, the decoder and the label predictor is written once here
(`_layer`, `_encoder`, `_audio_fwd`, `_chart_fwd`, `_decode_fwd`, `_label_predictor`) and runs with and without grad; latent_grad.py holds
only the backward.  What differs is where a buffer comes from, and that is the storage policy the forward is handed:
  `_Slots`  (no grad) named slots of a shape-keyed workspace, zero-filled when created and shared by a layer's blocks; the residual and
            the mixer write over their input (so the style head works on a copy of h); nothing is kept; `lengths=` and bf16x3 run here
  `_Tape`   (grad) a fresh tensor per request, the residual and the mixer write to a new one, and each block's tensors, the resampled
            streams and the heads' inputs are kept for the backward; SpecFeatures up to its SiLU is fp32 on the parameter itself, cast
            afterwards; a caller's own skip that would be read in place is cloned; `lengths=` and bf16x3 are refused
Tensors that outlive a call (skips, h, z, s, logits / chart, labels) are fresh allocations under both.
"""
from __future__ import annotations

import math
import weakref
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import latent_grad, ops
from ._lib import OD_ACT_NONE, OD_ACT_SILU
from .engine import Workspace

A_DIM = 72           # data/load_audio.py:11-15
X_DIM = 9            # data/beatmap/encode.py:14-29
N_HIT = 7            # HitSignals are channels 0..6 (encode.py:31-39)
NUM_LABELS = 5       # encode.py:50


@dataclass
class LayerArgs:                      # unet.py:9-13
    n_layers: int
    expand: int
    radius: int


@dataclass
class LatentModelArgs:                # latent/model.py:15-21
    h_dim: int
    ae_args: LayerArgs
    style_head_dim: int
    style_heads: int


def _ceil(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class _Node(nn.Module):
    pass


class _AudioEncoder(_Node):
    """`model.audio_encoder(audio)` — holds the reference's `audio_encoder.{0,1}.*` parameters."""

    def forward(self, audio: torch.Tensor, lengths: Optional[Sequence[int]] = None):
        return self._owner()._audio_encoder(audio, lengths)


def _shapes(emb_dim: int, style_dim: int, n_downs: int, stride: int, a: LatentModelArgs):
    """Every key of the reference's `LatentModel.state_dict()` -> (shape, init) in its order; init is
    'w' (default conv/linear init), 'b:<fan_in>' (bias), 'g:<gain>' (RMSNorm gamma) or 'z' (zero-initialised)."""
    D, L_ = a.h_dim, a.ae_args
    hf, k, ks = int(D * L_.expand * 2 / 3), 1 + 2 * L_.radius, 1 + 2 * (stride // 2)
    s: Dict[str, Tuple[tuple, str]] = {}

    def conv(name, shape, zero=False):
        fan = 1
        for n in shape[1:]:
            fan *= n
        s[name + ".weight"] = (shape, "z" if zero else "w")
        s[name + ".bias"] = ((shape[0],), "z" if zero else f"b:{fan}")

    def layer(p, cond_dim):
        for i in range(L_.n_layers):
            s[f"{p}norms.{i}.gamma"] = ((D,), "g:1.0")
        for i in range(L_.n_layers):
            b = f"{p}blocks.{i}."
            conv(b + "0.proj_vg.0", (D, 1, k))
            conv(b + "0.proj_vg.1", (2 * hf, D, 1))
            conv(b + "0.proj_o", (D, hf, 1))
            s[b + "1.gamma"] = ((D,), "g:0.001")
        s[p + "out_norm.gamma"] = ((D,), "g:1.0")
        if cond_dim > 0:
            for i in range(L_.n_layers):
                conv(f"{p}films.{i}", (3 * D, cond_dim), zero=True)

    def encoder(p):
        for i in range(n_downs):
            conv(f"{p}downs.{i}.0", (D, 1, ks))
        for i in range(n_downs):
            layer(f"{p}layers.{i}.", 0)

    conv("chart_encoder.0", (D, X_DIM, 1))
    encoder("chart_encoder.1.")
    conv("audio_encoder.0.net.1", (8, 1, 8, 3)); s["audio_encoder.0.net.2.gamma"] = ((8,), "g:1.0")
    conv("audio_encoder.0.net.4", (32, 8, 6, 3)); s["audio_encoder.0.net.5.gamma"] = ((32,), "g:1.0")
    conv("audio_encoder.0.net.8", (D, 32 * (A_DIM // 24), 1)); s["audio_encoder.0.net.9.gamma"] = ((D,), "g:1.0")
    encoder("audio_encoder.1.")
    layer("style_head.0.", 0)
    hd = a.style_head_dim * a.style_heads
    conv("style_head.1.scores", (a.style_heads, D, 1))
    conv("style_head.1.values", (hd, D, 1))
    conv("style_head.1.proj_out", (style_dim, hd))
    layer("temporal_layer.", style_dim)
    conv("temporal_head.0", (emb_dim, D, 1))
    conv("proj_emb", (D, emb_dim, 1))
    for i in range(n_downs):
        conv(f"decoder.ups.{i}.1", (D, 1, ks))
    for i in range(n_downs):
        layer(f"decoder.layers.{i}.", style_dim)
    for i in range(n_downs):
        m = f"decoder.mixers.{i}."
        conv(m + "proj.0", (D, D, 1)); s[m + "proj.1.gamma"] = ((D,), "g:1.0")
        conv(m + "gate", (D, D, 1), zero=True)
    conv("proj_out", (X_DIM, D, 1))
    conv("label_predictor.0", (D, style_dim))
    conv("label_predictor.2", (NUM_LABELS, D))
    return s


class _Slots:
    """Storage of a no-grad forward: every buffer is a named slot of one of the model's workspaces (zero-filled when created), so a
    layer's blocks share their six buffers; the residual and the mixer write over their input; nothing is kept.  Its counterpart with
    grad is latent_grad's `_Tape`."""
    fp32_front = False                      # SpecFeatures runs in the compute dtype, on the packed operand

    def __init__(self, ws: Workspace):
        self.buf = self.zeros = ws.get      # (name, shape, dtype)

    def over(self, x: torch.Tensor) -> torch.Tensor:
        """Where a kernel that may update x in place writes."""
        return x

    def fork(self, name: str, x: torch.Tensor) -> torch.Tensor:
        """What a layer may consume while x is still needed: a copy, because the layer updates its input in place."""
        t = self.buf(name, x.shape, x.dtype)
        t.copy_(x)
        return t

    def skip(self, i: int, sk: torch.Tensor, skf: torch.Tensor) -> torch.Tensor:
        return skf

    def record(self, **kept):
        pass


class LatentModel(nn.Module):
    def __init__(self, emb_dim: int, style_dim: int, n_downs: int, stride: int, args: LatentModelArgs):
        super().__init__()
        if isinstance(args, dict):
            args = LatentModelArgs(**args)
        if isinstance(args.ae_args, dict):
            args.ae_args = LayerArgs(**args.ae_args)
        self.emb_dim, self.style_dim, self.n_downs, self.stride, self.args = emb_dim, style_dim, n_downs, stride, args
        self.a_dim = args.h_dim
        self.chunk_size = stride ** n_downs
        D = args.h_dim
        if D < 8 or D > 512 or D & (D - 1):
            raise NotImplementedError("h_dim must be a power of two in 8..512 on the compiled path")
        if args.ae_args.radius not in (1, 2):
            raise NotImplementedError("depthwise kernel sizes 3 and 5 (radius 1, 2) are compiled")
        self.hf = int(D * args.ae_args.expand * 2 / 3)
        self.hp = _ceil(self.hf, 64)
        self.compute_dtype: Optional[torch.dtype] = None     # None: fp32 (bf16 when set)
        self.f32_matmul = "f32"                              # or "bf16x3", see DiffusionModel.f32_matmul
        for name, (shape, init) in _shapes(emb_dim, style_dim, n_downs, stride, args).items():
            t = torch.empty(*shape)
            if init == "w":
                fan = 1
                for n in shape[1:]:
                    fan *= n
                t.uniform_(-1 / math.sqrt(fan), 1 / math.sqrt(fan))
            elif init.startswith("b:"):
                bound = 1 / math.sqrt(int(init[2:]))
                t.uniform_(-bound, bound)
            elif init.startswith("g:"):
                t.fill_(float(init[2:]))
            else:
                t.zero_()
            self._register(name, nn.Parameter(t, requires_grad=False))
        object.__setattr__(self.audio_encoder, "_owner", weakref.ref(self))
        self._ws: Dict[tuple, Workspace] = {}
        self._packed: Dict[str, torch.Tensor] = {}
        self._packed_key = None
        self._packed_train = False
        self._plist: Optional[List[nn.Parameter]] = None
        self._rowmap = None
        self.register_load_state_dict_post_hook(lambda m, k: m.invalidate())

    def _register(self, dotted: str, p: nn.Parameter):
        node, parts = self, dotted.split(".")
        for i, part in enumerate(parts[:-1]):
            nxt = node._modules.get(part)
            if nxt is None:
                nxt = _AudioEncoder() if (i == 0 and part == "audio_encoder") else _Node()
                node.add_module(part, nxt)
            node = nxt
        node.register_parameter(parts[-1], p)

    # ------------------------------------------------------------------ plumbing
    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self.invalidate()
        return out

    def invalidate(self):
        """Forget packed GEMM operands and workspaces (call after editing parameters in place)."""
        self._packed, self._packed_key, self._packed_train, self._ws, self._plist = {}, None, False, {}, None

    def _params(self) -> List[nn.Parameter]:
        """The parameters, listed once (the constructor registers them all; invalidate() forgets the list)."""
        if self._plist is None:
            self._plist = list(self.parameters())
        return self._plist

    def P(self, name: str) -> torch.Tensor:
        return self.get_parameter(name)

    def _dtype(self) -> torch.dtype:
        return self.compute_dtype or torch.float32

    def _x3(self) -> bool:
        if self.f32_matmul not in ("f32", "bf16x3"):
            raise ValueError(f"f32_matmul must be 'f32' or 'bf16x3', got {self.f32_matmul!r}")
        return self.f32_matmul == "bf16x3"

    def _layer_prefixes(self) -> List[Tuple[str, bool]]:
        out = [(f"audio_encoder.1.layers.{i}.", False) for i in range(self.n_downs)]
        out += [(f"decoder.layers.{i}.", True) for i in range(self.n_downs)]
        out += [(f"chart_encoder.1.layers.{i}.", False) for i in range(self.n_downs)]
        return out + [("style_head.0.", False), ("temporal_layer.", True)]

    def _pack(self, dt: torch.dtype, train: bool = False) -> Dict[str, torch.Tensor]:
        """fp32 parameters -> GEMM operands of the compute dtype; SwiGLU width padded hf -> hp (zero rows/cols).  `train`: also the
        transposed operands the backward's data GEMMs read (name + ".T").  Once the grad path has packed, the cache follows the parameters:
        an optimizer edits them in place without calling invalidate(), which bumps their version counters, and those are then part of the
        key.  A model that never took the grad path does not look at them (in-place edits need invalidate(), as before)."""
        dev = self.P("proj_out.weight").device
        key = (dt, dev, tuple(p._version for p in self._params()) if train or self._packed_train else None)
        if self._packed_key == key and (self._packed_train or not train):
            return self._packed
        pk: Dict[str, torch.Tensor] = {}
        hf, hp = self.hf, self.hp
        rm = [-1] * (2 * hp)
        for j in range(hf):
            rm[j], rm[hp + j] = j, hf + j
        rowmap = torch.tensor(rm, dtype=torch.int32, device=dev)

        def pack(name, Np=None, Kp=None, rmap=None):
            w = self.P(name + ".weight")
            N, K = w.shape[0], w.numel() // w.shape[0]
            pk[name] = torch.empty(Np or N, Kp or K, dtype=dt, device=dev)
            ops.pack_weight(w, pk[name], row_map=rmap)
            if rmap is not None:
                pk[name + ".b"] = torch.empty(Np, dtype=torch.float32, device=dev)
                ops.pack_weight(self.P(name + ".bias"), pk[name + ".b"].view(Np, 1), row_map=rmap)
            # (the chart takes no gradient; the grad path runs SpecFeatures' projection in fp32 on the parameter itself)
            if train and name not in ("chart_encoder.0", "audio_encoder.0.net.8"):
                # N < 8 (the pool's scores): the gradient rows are padded to one 8-wide k chunk, like the chart's 9 channels forward
                pk[name + ".T"] = torch.empty(Kp or K, _ceil(Np or N, 8), dtype=dt, device=dev)
                ops.pack_weight(w, pk[name + ".T"], transpose=True, row_map=rmap)

        pack("audio_encoder.0.net.8")
        pack("chart_encoder.0", Kp=16)                      # 9 chart channels, zero-padded to one 16-wide k chunk
        pack("style_head.1.scores")
        pack("style_head.1.values")
        for p, _ in self._layer_prefixes():
            for i in range(self.args.ae_args.n_layers):
                pack(f"{p}blocks.{i}.0.proj_vg.1", Np=2 * hp, rmap=rowmap)
                pack(f"{p}blocks.{i}.0.proj_o", Kp=hp)
        for i in range(self.n_downs):
            pack(f"decoder.mixers.{i}.proj.0")
            pack(f"decoder.mixers.{i}.gate")
        self._packed, self._packed_key, self._packed_train = pk, key, train
        return pk

    def _workspace(self, tag: str, B: int, L: int, dt) -> Workspace:
        dev = self.P("proj_out.weight").device
        key = (tag, B, L, dt, dev)
        ws = self._ws.get(key)
        if ws is None:
            if len(self._ws) >= 8:
                self._ws.clear()
            ws = self._ws[key] = Workspace(dev)
        return ws

    def _check_lengths(self, lengths: Sequence[int], n: int, L: int, what: str) -> List[int]:
        lengths = [int(x) for x in lengths]
        if len(lengths) != n:
            raise ValueError(f"{what}: expected {n} lengths, got {len(lengths)}")
        for x in lengths:
            if x < self.chunk_size or x > L or x % self.chunk_size:
                raise ValueError(f"{what}: length {x} is not a multiple of chunk_size {self.chunk_size} in [{self.chunk_size}, {L}]")
        return lengths

    @staticmethod
    def _dev_i32(rows: List[List[int]], dev) -> torch.Tensor:
        """Host ints -> device int32, without waiting for the stream (pinned source, asynchronous copy)."""
        t = torch.tensor(rows, dtype=torch.int32)
        if dev.type != "cuda":
            return t.to(dev)
        return t.pin_memory().to(dev, non_blocking=True)

    def _level_lens(self, lengths: List[int], dev) -> torch.Tensor:
        """Frame-0 lengths (multiples of chunk_size) of B rows -> (n_downs + 1, B) device int32: row i = the lengths at level i."""
        return self._dev_i32([[x // self.stride ** i for x in lengths] for i in range(self.n_downs + 1)], dev)

    def _grad_path(self, *inputs) -> bool:
        """Gradients are wanted: grad mode is on and a parameter (`model.requires_grad_(True)`) or one of `inputs` requires grad."""
        return torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in inputs) or
                                            any(p.requires_grad for p in self._params()))

    # ------------------------------------------------------------------ the forward.  `st` is the storage policy (_Slots, or latent_grad's
    # _Tape); `lv` / `lens` are the device lengths of `lengths=` per level (None: dense); operands are packed by the caller (`_pack`).
    def _layer(self, st, tag: str, p: str, x: torch.Tensor, cond: Optional[torch.Tensor], B: int, L: int,
               outlive: bool = False, lens: Optional[torch.Tensor] = None):
        """unet.py:21-53.  x [B*L][D] through the blocks, then out_norm(x) into a buffer of `st` (`outlive`: into a tensor of its own, for
        the caller to hand on); returns it and the record `_Tape.layer_bwd` reads.  `lens` (device int32 [B]): row b is valid for frames < lens[b]; the depthwise convs stop there and the
        returned out_norm is 0 past it (everything else in a block is row-wise, so padded frames only ever affect themselves)."""
        M, D, dt, x3, pk = B * L, self.a_dim, x.dtype, self._x3(), self._packed
        k = 1 + 2 * self.args.ae_args.radius
        blocks = []
        for i in range(self.args.ae_args.n_layers):
            ssg = None
            if cond is not None:
                ssg = st.buf(f"{tag}.ssg{i}", (B, 3 * D), torch.float32)
                ops.linear_small(cond, self.P(f"{p}films.{i}.weight"), self.P(f"{p}films.{i}.bias"), ssg)
            b = f"{p}blocks.{i}.0."
            h = st.buf(tag + ".h", (M, D), dt)
            hd = st.buf(tag + ".hd", (M, D), dt)
            vg = st.buf(tag + ".vg", (M, 2 * self.hp), dt)
            hh = st.buf(tag + ".hh", (M, self.hp), dt)
            fo = st.buf(tag + ".fo", (M, D), dt)
            xo = st.over(x)
            inv = st.buf(tag + ".inv", (M,), torch.float32)
            ops.rmsnorm_affine_film(x, self.P(f"{p}norms.{i}.gamma"), ssg, h, B, L)
            ops.dwconv(h, self.P(b + "proj_vg.0.weight"), self.P(b + "proj_vg.0.bias"), hd, B, L, k, lens)
            ops.gemm_nt(hd, pk[b + "proj_vg.1"], pk[b + "proj_vg.1.b"], vg, x3=x3)
            ops.swiglu_rmsnorm(vg, hh, inv, self.hf, self.hp)
            ops.gemm_nt(hh, pk[b + "proj_o"], self.P(b + "proj_o.bias"), fo, x3=x3)
            ops.rmsnorm_affine_gate_residual(x, fo, self.P(f"{p}blocks.{i}.1.gamma"), ssg, xo, B, L)
            blocks.append((x, ssg, h, hd, vg, hh, inv, fo))
            x = xo
        out = torch.empty(M, D, dtype=dt, device=x.device) if outlive else st.buf(tag + ".out", (M, D), dt)
        ops.rmsnorm_affine_film(x, self.P(p + "out_norm.gamma"), None, out, B, L, lens=lens)
        return out, (p, blocks, x, cond, B, L)

    def _encoder(self, st, p: str, x: torch.Tensor, B: int, L: int, lv, outlive: bool):
        """unet.py:55-82.  Per level a layer, then the strided conv down: returns [(the layer's record, its output, Lo)], the last x and
        its frames per row.  `outlive`: the outputs and the last x are handed to the caller (audio_encoder's skips and h), so each is a
        tensor of its own, not a buffer of `st`."""
        D, dt, levels = self.a_dim, x.dtype, []
        for i in range(self.n_downs):
            y, rec = self._layer(st, f"l{i}", f"{p}layers.{i}.", x, None, B, L, outlive, lv[i])
            Lo = L // self.stride
            x = (torch.empty(B * Lo, D, dtype=dt, device=x.device) if outlive and i == self.n_downs - 1
                 else st.buf(f"x{i + 1}", (B * Lo, D), dt))
            ops.unet_down(y, self.P(f"{p}downs.{i}.0.weight"), self.P(f"{p}downs.{i}.0.bias"), x, B, Lo, self.stride, lv[i])
            levels.append((rec, y, Lo))
            L = Lo
        return levels, x, L

    def _head(self, x: torch.Tensor, name: str, B: int, L: int, n_sigmoid: int, rms: bool, lens) -> torch.Tensor:
        """x [B*L][D] -> (B, N, L) fp32 through the 1x1 conv `name`: sigmoid on the first n_sigmoid channels, or rms_norm over all."""
        W = self.P(name + ".weight")
        out = torch.empty(B, W.shape[0], L, dtype=torch.float32, device=x.device)
        ops.chart_head(x, W.view(W.shape[0], -1), self.P(name + ".bias"), out, B, L, n_sigmoid, rms=rms, lens=lens)
        return out

    def _audio_fwd(self, st, audio: torch.Tensor, lv=None):
        """latent/model.py:54.  audio (Ba, 72, L) fp32, contiguous -> the skips and h as (Ba, D, L_i) views of frame-major tensors of
        their own (they outlive the call)."""
        Ba, _, L = audio.shape
        dt, D, x3 = self._dtype(), self.a_dim, self._x3()
        lv = [None] * (self.n_downs + 1) if lv is None else lv
        # st.fp32_front: SpecFeatures stays fp32 in both modes, its 96 -> D projection included (the fp32 parameter is the GEMM operand): its
        # eight- and 32-element gradients are sums over every frame, where a rounded operand's error does not average out
        fdt = torch.float32 if st.fp32_front else dt
        p = "audio_encoder.0.net."
        f96 = st.buf("f96", (Ba * L, 32 * (A_DIM // 24)), fdt)
        ops.spec_features_conv(audio, *(self.P(p + n) for n in ("1.weight", "1.bias", "2.gamma", "4.weight", "4.bias", "5.gamma")), f96,
                               lens=lv[0])
        pre = st.buf("pre", (Ba * L, D), fdt)
        w8 = self.P(p + "8.weight").view(D, -1) if st.fp32_front else self._packed["audio_encoder.0.net.8"]
        ops.gemm_nt(f96, w8, self.P(p + "8.bias"), pre, x3=x3)
        x = st.buf("x0", (Ba * L, D), fdt)
        ops.rmsnorm_affine_film(pre, self.P(p + "9.gamma"), None, x, Ba, L, act=OD_ACT_SILU)
        if fdt != dt:
            x32, x = x, st.buf("x0c", (Ba * L, D), dt)
            ops.cast_rows(x32, x)
        levels, x, _ = self._encoder(st, "audio_encoder.1.", x, Ba, L, lv, outlive=True)
        st.record(audio=audio, Ba=Ba, L=L, f96=f96, pre=pre, levels=levels)
        return [skip.view(Ba, -1, D).permute(0, 2, 1) for _, skip, _ in levels], x.view(Ba, -1, D).permute(0, 2, 1)

    def _chart_fwd(self, st, chart: torch.Tensor, lv=None):
        """latent/model.py:93-101.  chart (B, 9, L) fp32, contiguous -> z (B, emb_dim, L / chunk_size), s (B, style_dim): chart encoder,
        style head (layer + AttnPool + rms_norm), temporal layer / head."""
        B, _, L = chart.shape
        dt, D, x3, pk = self._dtype(), self.a_dim, self._x3(), self._packed
        lv = [None] * (self.n_downs + 1) if lv is None else lv
        cf = self._frames(chart, dt, st.zeros("cf", (B * L, 16), dt))      # columns 9..15 stay zero
        x = st.buf("x0", (B * L, D), dt)
        ops.gemm_nt(cf, pk["chart_encoder.0"], self.P("chart_encoder.0.bias"), x, x3=x3)
        levels, h, Li = self._encoder(st, "chart_encoder.1.", x, B, L, lv, outlive=False)
        ll = lv[self.n_downs]                                 # h is [B*l][D]; both heads below read it
        # style head: layer -> AttnPool -> rms_norm (no gain)
        ys, rec_s = self._layer(st, "sh", "style_head.0.", st.fork("hs", h), None, B, Li, lens=ll)
        heads, hd = self.args.style_heads, self.args.style_head_dim
        sc = st.buf("sc", (B * Li, heads), dt)
        va = st.buf("va", (B * Li, heads * hd), dt)
        ops.gemm_nt(ys, pk["style_head.1.scores"], self.P("style_head.1.scores.bias"), sc, x3=x3)
        ops.gemm_nt(ys, pk["style_head.1.values"], self.P("style_head.1.values.bias"), va, x3=x3)
        pooled = st.buf("pooled", (B, heads * hd), torch.float32)
        ops.attn_pool(sc, va, pooled, B, Li, heads, hd, ll)
        s_pre = st.buf("s_pre", (B, self.style_dim), torch.float32)
        ops.linear_small(pooled, self.P("style_head.1.proj_out.weight"), self.P("style_head.1.proj_out.bias"), s_pre)
        s = torch.empty(B, self.style_dim, dtype=torch.float32, device=chart.device)
        ops.rmsnorm_rows(s_pre, None, s, 1e-6)
        # temporal layer (FiLM from s) -> Conv1d(D -> emb_dim) -> rms_norm over the emb_dim channels
        yt, rec_t = self._layer(st, "tl", "temporal_layer.", h, s, B, Li, lens=ll)
        z = self._head(yt, "temporal_head.0", B, Li, 0, True, ll)
        st.record(B=B, L=L, l=Li, cf=cf, levels=levels, ys=ys, rec_s=rec_s, sc=sc, va=va, pooled=pooled, s_pre=s_pre, s=s, yt=yt, rec_t=rec_t)
        return z, s

    def _decode_fwd(self, st, z: torch.Tensor, s: torch.Tensor, skips, n_sigmoid: int, lv=None, prow=None, songs: Optional[int] = None):
        """latent/model.py:103-114.  z (B, E, l), s (B, style_dim) fp32, contiguous -> (B, 9, L) with a sigmoid on the first n_sigmoid
        channels.  Varlen: skip row prow[b] (device int32 [B]) of `songs` rows serves decoder row b."""
        skips = list(skips)
        if len(skips) != self.n_downs:
            raise ValueError(f"expected {self.n_downs} skips, got {len(skips)}")
        B, E, l = z.shape
        dt, D, x3, pk = self._dtype(), self.a_dim, self._x3(), self._packed
        lv = [None] * (self.n_downs + 1) if lv is None else lv
        x = st.buf("x0", (B * l, D), dt)
        ops.proj_in(z, self.P("proj_emb.weight").view(D, E), self.P("proj_emb.bias"), x)
        ups, Li = [], l
        for i in range(self.n_downs):
            Lu = Li * self.stride
            lvl = self.n_downs - i                                # level of x; xu is at level lvl - 1
            sk = skips[lvl - 1]
            Bs = sk.shape[0]
            if sk.shape[1] != D or sk.shape[2] != Lu or (Bs not in (1, B) if songs is None else Bs != songs):
                raise ValueError(f"skip {tuple(sk.shape)} does not match ({f'{B}|1' if songs is None else f'G = {songs}'}, {D}, {Lu})")
            bc = Bs == 1 and B > 1
            xu = st.buf(f"xu{i}", (B * Lu, D), dt)
            ops.unet_up(x, self.P(f"decoder.ups.{i}.1.weight"), self.P(f"decoder.ups.{i}.1.bias"), xu, B, Li, self.stride, lv[lvl])
            skf = st.skip(lvl - 1, sk, self._frames(sk, dt))
            m = f"decoder.mixers.{i}."
            pr = st.buf(f"pr{i}", (Bs * Lu, D), dt)
            ops.gemm_nt(skf, pk[m + "proj.0"], self.P(m + "proj.0.bias"), pr, x3=x3)
            gx = st.buf(f"gx{i}", (B * Lu, D), dt)
            ops.gemm_nt(xu, pk[m + "gate"], self.P(m + "gate.bias"), gx, x3=x3)
            xm = st.over(xu)
            ops.unet_mixer(xu, pr, bc, gx, self.P(m + "proj.1.gamma"), xm, B, Lu, prow=prow)
            y, rec = self._layer(st, f"l{i}", f"decoder.layers.{i}.", xm, s, B, Lu, lens=lv[lvl - 1])
            ups.append((x, xu, skf, pr, gx, bc, Bs, rec, Li))
            x, Li = y, Lu
        st.record(z=z, s=s, B=B, l=l, ups=ups, x_out=x, Lout=Li)
        return self._head(x, "proj_out", B, Li, n_sigmoid, False, lv[0])

    def _label_predictor(self, s: torch.Tensor, tape=None) -> torch.Tensor:
        """latent/model.py:72-76.  s (B, style_dim) fp32, contiguous.  With a tape the hidden layer's pre-activation is stored too."""
        B = s.shape[0]
        hid = torch.empty(B, self.a_dim, dtype=torch.float32, device=s.device)
        pre = None if tape is None else torch.empty_like(hid)
        out = torch.empty(B, NUM_LABELS, dtype=torch.float32, device=s.device)
        ops.linear_small(s, self.P("label_predictor.0.weight"), self.P("label_predictor.0.bias"), hid, pre, OD_ACT_SILU)
        ops.linear_small(hid, self.P("label_predictor.2.weight"), self.P("label_predictor.2.bias"), out)
        if tape is not None:
            tape.record(s=s, hid=hid, hid_pre=pre)
        return out

    def _frames(self, t: torch.Tensor, dt: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(B, C, L) tensor -> frame-major [B*L][C] of the compute dtype; free for the views audio_encoder returns.  With `out`
        ([B*L][>= C] of dt) the first C columns of it are written."""
        B, C, L = t.shape
        if out is None:
            fm = t.permute(0, 2, 1)
            if fm.is_contiguous() and t.dtype == dt:
                return fm.reshape(B * L, C)
            out = torch.empty(B * L, C, dtype=dt, device=t.device)
        ops.cl_to_frames(t.detach().to(torch.float32).contiguous(), out)
        return out

    # ------------------------------------------------------------------ the calls: checks, then the no-grad forward in the model's
    # workspaces, or latent_grad's autograd Functions around the same forward
    def _audio_encoder(self, audio: torch.Tensor, lengths: Optional[Sequence[int]] = None):
        if not self._grad_path():                     # (the spectrogram itself takes no gradient)
            return self._audio_encoder_nograd(audio, lengths)
        if lengths is not None:
            raise NotImplementedError("audio_encoder: `lengths=` (varlen) is an inference form; the grad path takes dense batches")
        if audio.dim() != 3 or audio.shape[1] != A_DIM or audio.shape[2] % self.chunk_size:
            raise ValueError(f"audio must be (B, {A_DIM}, L) with L a multiple of chunk_size {self.chunk_size}, got {tuple(audio.shape)}")
        return latent_grad.audio_encoder(self, audio)

    @torch.no_grad()
    def _audio_encoder_nograd(self, audio: torch.Tensor, lengths: Optional[Sequence[int]] = None):
        """`lengths` (one per row, multiples of chunk_size): row g of audio holds a song of lengths[g] frames, zero-padded to L; the skips
        and h are then 0 past each song's length at every level."""
        audio = audio.detach().to(torch.float32).contiguous()
        Ba, F, L = audio.shape
        if F != A_DIM:
            raise ValueError(f"audio must have {A_DIM} spectrogram bins, got {F}")
        if L % self.chunk_size:
            raise ValueError(f"audio length {L} is not a multiple of chunk_size {self.chunk_size} (pad_to_multiple first)")
        lv = None if lengths is None else self._level_lens(self._check_lengths(lengths, Ba, L, "audio_encoder"), audio.device)
        dt = self._dtype()
        self._pack(dt)
        return self._audio_fwd(_Slots(self._workspace("enc", Ba, L, dt)), audio, lv)

    @torch.no_grad()
    def _decode(self, z, s, audio, skips, n_sigmoid: int, lengths=None, offs=None):
        if lengths is None and offs is not None:
            raise ValueError("decode: `offs` goes with `lengths`")
        if skips is None:
            if audio is None:
                raise ValueError("decode needs `audio` or `skips`")
            skips, _ = self._audio_encoder_nograd(audio, lengths)
        z = z.detach().to(torch.float32).contiguous()
        s = s.detach().to(torch.float32).contiguous()
        B, E, l = z.shape
        dt = self._dtype()
        self._pack(dt)
        lv = prow = G = None
        if lengths is not None:
            # varlen: song g = rows offs[g]:offs[g+1] of z / s, skips[i] row g; lengths[g] in chart frames
            G = len(lengths)
            offs = list(range(G + 1)) if offs is None else [int(o) for o in offs]
            if len(offs) != G + 1 or offs[0] != 0 or offs[-1] != B or any(offs[g + 1] <= offs[g] for g in range(G)):
                raise ValueError(f"decode: offs must rise from 0 to B = {B} in G + 1 = {G + 1} steps, got {offs}")
            lengths = self._check_lengths(lengths, G, l * self.chunk_size, "decode")
            rows = [g for g in range(G) for _ in range(offs[g + 1] - offs[g])]
            lv = self._level_lens([lengths[g] for g in rows], z.device)
            prow = self._dev_i32(rows, z.device)
        ws = self._workspace("dec" if lv is None else f"dec.vl{G}", B, l, dt)
        return self._decode_fwd(_Slots(ws), z, s, skips, n_sigmoid, lv, prow, G), s

    def decode_logits(self, z, s, *, audio=None, skips=None, lengths=None, offs=None) -> torch.Tensor:
        if not self._grad_path(z, s, *(skips or ())):
            return self._decode(z, s, audio, skips, n_sigmoid=0, lengths=lengths, offs=offs)[0]
        if lengths is not None or offs is not None:
            raise NotImplementedError("decode_logits: `lengths=` (varlen) is an inference form; the grad path takes dense batches")
        if skips is None:
            if audio is None:
                raise ValueError("decode needs `audio` or `skips`")
            skips, _ = self._audio_encoder(audio)
        return latent_grad.decode_logits(self, z, s, skips)

    @torch.no_grad()
    def decode(self, z, s, *, audio=None, skips=None, lengths=None, offs=None):
        """(chart, labels): sigmoid on the hit signals, cursor signals raw, labels clamped to [0, 10]
        (latent/model.py:116-134).  Varlen: `lengths` (G songs, chart frames, multiples of chunk_size), `offs` (G + 1 row offsets of
        z / s, default one row per song) and skips / audio with one row per song; the chart is 0 past each song's length."""
        chart, s32 = self._decode(z, s, audio, skips, n_sigmoid=N_HIT, lengths=lengths, offs=offs)
        return chart, self._label_predictor(s32).clamp_(0, 10)

    def forward(self, audio, z, s):                                          # latent/model.py:78-91
        if self._grad_path(z, s):
            return self.decode_logits(z, s, audio=audio), latent_grad.label_predictor(self, s)
        with torch.no_grad():
            return self.decode_logits(z, s, audio=audio), self._label_predictor(s.detach().to(torch.float32).contiguous())

    def encode_chart(self, chart: torch.Tensor, lengths: Optional[Sequence[int]] = None):
        if not self._grad_path():                     # (the chart itself takes no gradient)
            return self._encode_chart_nograd(chart, lengths)
        if lengths is not None:
            raise NotImplementedError("encode_chart: `lengths=` (varlen) is an inference form; the grad path takes dense batches")
        if chart.dim() != 3 or chart.shape[1] != X_DIM or chart.shape[2] % self.chunk_size:
            raise ValueError(f"chart must be (B, {X_DIM}, L) with L a multiple of chunk_size {self.chunk_size}, got {tuple(chart.shape)}")
        return latent_grad.encode_chart(self, chart)

    @torch.no_grad()
    def _encode_chart_nograd(self, chart: torch.Tensor, lengths: Optional[Sequence[int]] = None):
        """The dataset-encoding direction (scripts/encode_latents.py).  `lengths` (one per map, multiples of chunk_size): map b holds
        lengths[b] frames; z is 0 past lengths[b] / chunk_size and s pools over the map's own frames."""
        chart = chart.detach().to(torch.float32).contiguous()
        B, X, L = chart.shape
        if X != X_DIM:
            raise ValueError(f"chart must have {X_DIM} signals, got {X}")
        if L % self.chunk_size:
            raise ValueError(f"chart length {L} is not a multiple of chunk_size {self.chunk_size} (pad_to_multiple first)")
        lv = None if lengths is None else self._level_lens(self._check_lengths(lengths, B, L, "encode_chart"), chart.device)
        dt = self._dtype()
        self._pack(dt)
        return self._chart_fwd(_Slots(self._workspace("chart", B, L, dt)), chart, lv)

