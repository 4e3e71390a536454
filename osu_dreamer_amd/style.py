"""`StyleModel` inference on the HIP path — the step before `diffusion.sample` in `LDM.sample`
(osu_dreamer/models/inference/model.py:49; reference model: osu_dreamer/models/style/model.py:29-119).

Same constructor, state-dict keys (`rff.W`, `rff.b` buffers included), `forward(st, labels) -> (u, v)`,
`compute_conditioning(labels)` and `sample(labels, num_steps=16)`.  The conditioning and every FiLM
(`films[i](c)`) depend only on the labels, so `sample` computes them once instead of on each of its
`num_steps + 1` evaluations; the step body is captured into a hipGraph like the denoiser's.  `sample_many(labels_list)`
samples several songs' label batches as one evaluation batch, each song with its own step size.

Training (osu_dreamer/models/style/train.py): the parameters are views of one `ParamArena` with a twin gradient buffer, as the
denoiser's are, so `FusedAdamWEMA(style, ema=...)` steps them in one pass.  `train_forward` keeps the activations the backward reads in
a workspace keyed by (B, dtype); `train_backward` launches the backward kernels, which write straight into `arena.grad`.  Models are
built frozen (`requires_grad_(False)`); `StyleTrainer` un-freezes its own.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import det, ops
from ._lib import OD_ACT_NONE, OD_ACT_SILU
from .model import ParamArena

NUM_LABELS = 5
FP32_EPS = float(torch.finfo(torch.float32).eps)


@dataclass
class StyleModelArgs:
    label_features: int
    h_dim: int
    depth: int
    expand: int
    dropout: float = 0.


class _Node(nn.Module):
    pass


class StyleModel(nn.Module):
    def __init__(self, style_dim: int, args: StyleModelArgs):
        super().__init__()
        if isinstance(args, dict):
            args = StyleModelArgs(**args)
        self.style_dim, self.args = style_dim, args
        d0_sq = 2.0 * style_dim
        t99 = torch.tensor(2.3263478740408408).sigmoid().item()
        self.c0 = (1 - t99) ** 2 * d0_sq
        self.u_scale = math.sqrt(d0_sq)
        self.use_graph = True
        H, F, S = args.h_dim, args.label_features, style_dim

        def P(*shape, std=None):
            t = torch.empty(*shape)
            fan = shape[-1] if len(shape) > 1 else shape[0]
            return t.normal_(0, std if std is not None else 1.0 / math.sqrt(fan))

        self.rff = _Node()
        self.rff.register_buffer("W", torch.randn(F, 1) * 32.0)              # FourierFeatures(1, F, n_bins=32)
        self.rff.register_buffer("b", torch.empty(F).uniform_(-math.pi, math.pi))
        init: List[Tuple[str, torch.Tensor]] = [
            ("cond_proj_w", P(NUM_LABELS, F, H, std=math.sqrt(2.0 / (F + H)))),
            ("cond_proj_b", torch.zeros(NUM_LABELS, H)),
            ("null_labels", P(NUM_LABELS, H, std=H ** -0.5)),
            ("proj_in.weight", P(H, S)), ("proj_in.bias", torch.zeros(H)),
            ("proj_out.0.weight", torch.ones(H)),
            ("proj_out.1.weight", torch.zeros(S, H)), ("proj_out.1.bias", torch.zeros(S)),
            ("u_out.weight", torch.zeros(1, H)), ("u_out.bias", torch.full((1,), -0.4328)),
        ]
        films = [(f"films.{i}.weight", torch.zeros(3 * H, H), f"films.{i}.bias", torch.zeros(3 * H)) for i in range(args.depth)]
        blocks = []
        for i in range(args.depth):
            blocks += [(f"blocks.{i}.0.weight", P(args.expand * H, H)), (f"blocks.{i}.0.bias", torch.zeros(args.expand * H)),
                       (f"blocks.{i}.3.weight", P(H, args.expand * H)), (f"blocks.{i}.3.bias", torch.zeros(H))]
        for wn, w, bn, b in films:
            init += [(wn, w), (bn, b)]
        init += blocks
        # every parameter is a view of one flat fp32 arena (+ a twin for gradients): one optimizer / EMA / norm pass over one buffer
        self._inventory = [(n, tuple(t.shape), "") for n, t in init]
        self.arena = ParamArena(self._inventory)
        for n, t in init:
            self.arena.view(n).copy_(t)
        self.compute_dtype: Optional[torch.dtype] = None                 # None: follow autocast, else fp32
        self._register_views()
        self.requires_grad_(False)
        self._buf: Dict[str, torch.Tensor] = {}
        self._buf_gen = 0          # bumped on every (re)allocation: a captured graph holding old addresses is stale
        self._tws: Dict[tuple, Dict[str, torch.Tensor]] = {}             # training workspaces, keyed by (B, dtype, device)
        self._tkey = None

    # ---- parameter plumbing (as DiffusionModel's) ----------------------------------------
    def _register_views(self):
        for name, _, _ in self._inventory:
            parts = name.split(".")
            mod = self
            for part in parts[:-1]:
                if part not in mod._modules:
                    mod.add_module(part, _Node())
                mod = mod._modules[part]
            old = mod._parameters.get(parts[-1])
            mod._parameters[parts[-1]] = nn.Parameter(self.arena.view(name), requires_grad=True if old is None else old.requires_grad)

    def _apply(self, fn, recurse=True):
        """`.to()/.cuda()/.float()` move the arena as a whole and re-create the views; the two rff buffers move as buffers do."""
        new = fn(self.arena.data)
        if new.dtype != torch.float32:
            raise TypeError("StyleModel keeps fp32 master parameters; use compute_dtype / autocast for bf16")
        if new is not self.arena.data:
            self.arena.data = new.contiguous()
            self.arena.grad = None
            self._register_views()
            self._tws, self._tkey = {}, None
        for k, b in list(self.rff._buffers.items()):
            self.rff._buffers[k] = fn(b)
        return self

    def attach_grads(self):
        """Point every parameter's .grad at its slice of the arena's grad buffer (zeroing it if any .grad was dropped)."""
        g = self.arena.ensure_grad()
        fresh = False
        for name, p in self.named_parameters():
            gv = self.arena.grad_view(name)
            if p.grad is None or p.grad.data_ptr() != gv.data_ptr():
                p.grad = gv
                fresh = True
        if fresh:
            g.zero_()
        return g

    def adopt_grads(self):
        """Before an optimizer step: make the arena's gradient buffer hold what every parameter's `.grad` says (a no-op when they are the
        same memory, which attach_grads arranges)."""
        g = self.arena.ensure_grad()
        for name, p in self.named_parameters():
            gv = self.arena.grad_view(name)
            if p.grad is None:
                gv.zero_()
                p.grad = gv
            elif p.grad.data_ptr() != gv.data_ptr():
                gv.copy_(p.grad.reshape(gv.shape))
                p.grad = gv
        return g

    def _dtype(self) -> torch.dtype:
        if self.compute_dtype is not None:
            return self.compute_dtype
        dev = self.arena.data.device.type
        if torch.is_autocast_enabled(dev) and torch.get_autocast_dtype(dev) == torch.bfloat16:
            return torch.bfloat16
        return torch.float32

    # ------------------------------------------------------------------
    def _b(self, name, shape, like, dtype=torch.float32):
        t = self._buf.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.device != like.device or t.dtype != dtype:
            t = torch.zeros(shape, dtype=dtype, device=like.device)
            self._buf[name] = t
            self._buf_gen += 1
        return t

    def _w(self):
        return {k: v.detach() for k, v in self.state_dict().items()}

    def compute_conditioning(self, labels: torch.Tensor) -> torch.Tensor:
        labels = labels.detach().float().contiguous()
        W = self._w()
        c = self._b("c", (labels.shape[0], self.args.h_dim), labels)
        ops.style_conditioning(labels, W["rff.W"].contiguous(), W["rff.b"], W["cond_proj_w"], W["cond_proj_b"],
                               W["null_labels"], c)
        return c

    def _films(self, c, W):
        B, H = c.shape
        out = []
        for i in range(self.args.depth):
            ssg = self._b(f"ssg.{i}", (B, 3 * H), c)
            ops.linear_small(c, W[f"films.{i}.weight"], W[f"films.{i}.bias"], ssg)
            out.append(ssg)
        return out

    def _eval(self, st, ssgs, W, u, v):
        """One network evaluation given the (label-only) FiLM tensors."""
        B, H, a = st.shape[0], self.args.h_dim, self.args
        x, h = self._b("x", (B, H), st), self._b("h", (B, H), st)
        h1, h2 = self._b("h1", (B, a.expand * H), st), self._b("h2", (B, H), st)
        inv = self._b("inv", (B,), st)
        ops.linear_small(st, W["proj_in.weight"], W["proj_in.bias"], x)
        for i in range(a.depth):
            ops.rmsnorm_film(x, ssgs[i], None, False, h, inv, B, 1)
            ops.linear_small(h, W[f"blocks.{i}.0.weight"], W[f"blocks.{i}.0.bias"], h1, None, OD_ACT_SILU)
            ops.linear_small(h1, W[f"blocks.{i}.3.weight"], W[f"blocks.{i}.3.bias"], h2)
            ops.rmsnorm_gate_residual(x, h2, ssgs[i], x, inv, B, 1)
        xn = self._b("xn", (B, H), st)
        ops.rmsnorm_rows(x, W["proj_out.0.weight"], xn, FP32_EPS)
        ops.linear_small(xn, W["proj_out.1.weight"], W["proj_out.1.bias"], v)
        ops.rmsnorm_rows(x, None, xn, 1e-6)
        zero_mod = self._b("zero_mod", (B, 2 * H), st)
        ops.uhead_tail(xn, zero_mod, W["u_out.weight"], W["u_out.bias"], u, 1, self.u_scale)

    # ---- training forward / backward (style/model.py:82-100 and its autograd) --------------
    # Products.  fp32: exact fp32 throughout — od_linear_small[_bwd] below `gemm_min_rows` batch rows, the fp32 MFMA chain of
    # od_gemm_nt / od_gemm_tn from there on (at B = 512 it is 2-3 x faster on every product class of the step, the narrow ones included:
    # profiles/r09_style_train.txt).  bf16: the block linears are bf16 od_gemm_nt / od_gemm_tn products with fp32 accumulation over a
    # bf16 activation stream, as autocast runs them, at any batch size; proj_in, the FiLM linears (their output is the fp32 modulation
    # the norm kernels read), proj_out and the u-head stay fp32 as above, with od_cast_rows at the two boundaries.  Norm statistics, the
    # loss and the master weights are fp32 in both.
    gemm_min_rows = 64

    def _train_ws(self, B: int, dt: torch.dtype, dev) -> Dict[str, torch.Tensor]:
        key = (B, dt, dev)
        ws = self._tws.get(key)
        if ws is None:
            a, H, S = self.args, self.args.h_dim, self.style_dim
            X = a.expand * H
            z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
            za = lambda *shape: torch.zeros(*shape, dtype=dt, device=dev)          # the activation stream
            ws = {"labels": z(B, NUM_LABELS), "st": z(B, S), "c": z(B, H), "dc": z(B, H), "x": za(a.depth + 1, B, H),
                  "inv1": z(a.depth, B), "inv2": z(a.depth, B), "ssg": z(a.depth, B, 3 * H), "dssg": z(B, 3 * H),
                  "pre": za(a.depth, B, X), "h2": za(a.depth, B, H), "h": za(B, H), "h1": za(B, X),
                  "dh1": za(B, X), "dpre": z(B, max(a.expand, 3) * H), "dpre_a": za(B, X), "dh": za(B, H), "dh2": za(B, H), "dx": za(B, H),
                  "xl": z(B, H), "dxl": z(B, H),
                  "xn_v": z(B, H), "xn_u": z(B, H), "dxn": z(B, H), "dfm": z(B, H), "zero_mod": z(B, 2 * H), "dmod": z(B, 2 * H)}
            self._tws[key] = ws
        self._tkey = key
        return ws

    def _det_flush(self, *tensors, register: bool = False):
        """OD_DETERMINISTIC: fold the integer shadows of these atomically-accumulated buffers into them, before their first reader
        (`register`: make them accumulation targets first; idempotent).  No-op unless the mode is on."""
        ctx = det.context(self.arena.data.device)
        if ctx is not None:
            for t in tensors:
                if register:
                    ctx.register(t)
                else:
                    ctx.flush(t)

    def _packed(self, ws, name: str, dt: torch.dtype, transpose: bool) -> torch.Tensor:
        """The weight `name` as a GEMM operand of type dt ([N, K], or [K, N] when transposed: what backward-data reads), re-packed from
        the master on every call (the masters move at every optimizer step).  The fp32 un-transposed operand is the master itself."""
        w = self.arena.view(name + ".weight")
        if dt == torch.float32 and not transpose:
            return w
        key = ("WT." if transpose else "W.") + name
        buf = ws.get(key)
        if buf is None:
            N, K = w.shape
            buf = ws[key] = torch.empty((K, N) if transpose else (N, K), dtype=dt, device=w.device)
        ops.pack_weight(w, buf, transpose=transpose)
        return buf

    def _gemm32(self, B: int, N: int, K: int) -> bool:
        return B >= self.gemm_min_rows and N % 4 == 0 and K % 4 == 0

    def _linear_f32(self, ws, name: str, x, out):
        """out = x W^T + b in exact fp32 (proj_in, films.i, proj_out.1)."""
        w, b = self.arena.view(name + ".weight"), self.arena.view(name + ".bias")
        if self._gemm32(x.shape[0], w.shape[0], w.shape[1]):
            ops.gemm_nt(x, w, b, out)
        else:
            ops.linear_small(x, w, b, out)

    def _linear_f32_bwd(self, ws, name: str, x, dout, dx, accumulate_dx: bool = False):
        """dW += , db += and dx (+)= of `_linear_f32` (dx may be None)."""
        w, G = self.arena.view(name + ".weight"), self.arena.grad_view
        B, N = dout.shape
        if self._gemm32(B, N, w.shape[1]):
            ops.gemm_tn(dout, x, G(name + ".weight"), dbias=G(name + ".bias"))
            if dx is not None:
                ops.gemm_nt(dout, self._packed(ws, name, torch.float32, True), None, dx, accumulate=accumulate_dx)
        else:
            ops.linear_small_bwd(x, w, None, dout, ws["dpre"].view(-1)[:B * N].view(B, N), G(name + ".weight"), G(name + ".bias"), dx,
                                 accumulate_dx)

    def train_forward(self, st: torch.Tensor, labels: torch.Tensor, u: torch.Tensor, v: torch.Tensor):
        """(u, v) = forward(st, labels), keeping what `train_backward` reads: per layer x, inv_rms, the pre-activation of blocks.i.0, h2 and
        its inv_rms, and the label-only c and FiLM tensors (computed once, for all layers).  st (B, S) and labels (B, 5) are fp32."""
        a = self.args
        if a.dropout != 0 and self.training:
            raise NotImplementedError("StyleModel training with dropout != 0 (nn.Dropout at osu_dreamer/models/style/model.py:67) is not "
                                      "implemented; the reference's model.yml never sets it")
        dt = self._dtype()
        f32 = dt == torch.float32
        if not f32 and (a.h_dim % 8 or (a.expand * a.h_dim) % 8):
            raise ValueError("the bf16 style step needs h_dim to be a multiple of 8 (od_gemm_nt's operand alignment)")
        B, H, X = st.shape[0], a.h_dim, a.expand * a.h_dim
        ws, W = self._train_ws(B, dt, st.device), self._w()
        ws["labels"].copy_(labels)
        ws["st"].copy_(st)
        ops.style_conditioning(ws["labels"], W["rff.W"].contiguous(), W["rff.b"], W["cond_proj_w"], W["cond_proj_b"], W["null_labels"], ws["c"])
        for i in range(a.depth):
            self._linear_f32(ws, f"films.{i}", ws["c"], ws["ssg"][i])
        x = ws["x"]
        if f32:
            self._linear_f32(ws, "proj_in", ws["st"], x[0])
        else:
            self._linear_f32(ws, "proj_in", ws["st"], ws["xl"])
            ops.cast_rows(ws["xl"], x[0])
        blocks_gemm = not f32 or self._gemm32(B, X, H)
        for i in range(a.depth):
            n0, n3 = f"blocks.{i}.0", f"blocks.{i}.3"
            ops.rmsnorm_film(x[i], ws["ssg"][i], None, False, ws["h"], ws["inv1"][i], B, 1)
            if blocks_gemm:
                ops.gemm_nt(ws["h"], self._packed(ws, n0, dt, False), W[n0 + ".bias"], ws["pre"][i])
                ops.silu(ws["pre"][i], ws["h1"])
                ops.gemm_nt(ws["h1"], self._packed(ws, n3, dt, False), W[n3 + ".bias"], ws["h2"][i])
            else:
                ops.linear_small(ws["h"], W[n0 + ".weight"], W[n0 + ".bias"], ws["h1"], ws["pre"][i], OD_ACT_SILU)
                ops.linear_small(ws["h1"], W[n3 + ".weight"], W[n3 + ".bias"], ws["h2"][i])
            ops.rmsnorm_gate_residual(x[i], ws["h2"][i], ws["ssg"][i], x[i + 1], ws["inv2"][i], B, 1)
        if f32:
            xl = x[a.depth]
        else:
            xl = ws["xl"]
            ops.cast_rows(x[a.depth], xl)
        ops.rmsnorm_rows(xl, W["proj_out.0.weight"], ws["xn_v"], FP32_EPS)
        self._linear_f32(ws, "proj_out.1", ws["xn_v"], v)
        ops.rmsnorm_rows(xl, None, ws["xn_u"], 1e-6)
        ops.uhead_tail(ws["xn_u"], ws["zero_mod"], W["u_out.weight"], W["u_out.bias"], u, 1, self.u_scale)

    def train_backward(self, du: torch.Tensor, dv: torch.Tensor):
        """Parameter gradients of the last `train_forward` under du (B,), dv (B, S): accumulated (+=) into `arena.grad`."""
        a, ar = self.args, self.arena
        B, dt, _ = self._tkey
        f32 = dt == torch.float32
        H, X = a.h_dim, a.expand * a.h_dim
        ws, W = self._tws[self._tkey], self._w()
        G = ar.grad_view
        blocks_gemm = not f32 or self._gemm32(B, X, H)
        # the buffers this backward accumulates into with fp32 atomics (od_linear_small_bwd's dx slices, od_uhead_tail_bwd's and
        # od_gemm_tn's weight gradients): integer shadows in the deterministic mode
        atomic_dx = [ws["dxn"], ws["dc"]] + ([] if blocks_gemm else [ws["dh1"], ws["dh"]])
        self._det_flush(ar.ensure_grad(), *atomic_dx, register=True)
        scratch = lambda n: ws["dpre"].view(-1)[:B * n].view(B, n)                  # od_linear_small_bwd's fp32 workspace
        x, dx = ws["x"], ws["dx"]
        xl, dxl = (x[a.depth], dx) if f32 else (ws["xl"], ws["dxl"])             # (bf16: xl still holds the fp32 copy of the last x)
        self._linear_f32_bwd(ws, "proj_out.1", ws["xn_v"], dv, ws["dxn"])
        self._det_flush(ws["dxn"])
        ops.rmsnorm_rows_bwd(xl, W["proj_out.0.weight"], ws["dxn"], dxl, G("proj_out.0.weight"), FP32_EPS, False)
        ops.uhead_tail_bwd(ws["xn_u"], ws["zero_mod"], W["u_out.weight"], W["u_out.bias"], du, ws["dfm"], ws["dmod"], G("u_out.weight"),
                           G("u_out.bias"), 1, self.u_scale)
        ops.rmsnorm_rows_bwd(xl, None, ws["dfm"], dxl, None, 1e-6, True)
        if not f32:
            ops.cast_rows(dxl, dx)
        dssg = ws["dssg"]
        for i in reversed(range(a.depth)):
            n0, n3 = f"blocks.{i}.0", f"blocks.{i}.3"
            ssg = ws["ssg"][i]
            dssg.zero_()
            ops.rmsnorm_gate_residual_bwd(ws["h2"][i], ws["inv2"][i], ssg, dx, ws["dh2"], dssg, B, 1)
            ops.silu(ws["pre"][i], ws["h1"])                                              # h1 and h are recomputed, not kept
            ops.rmsnorm_film(x[i], ssg, None, False, ws["h"], ws["inv1"][i], B, 1)
            if blocks_gemm:
                ops.gemm_tn(ws["dh2"], ws["h1"], G(n3 + ".weight"), dbias=G(n3 + ".bias"))
                ops.gemm_nt(ws["dh2"], self._packed(ws, n3, dt, True), None, ws["dh1"])
                ops.silu_bwd(ws["pre"][i], ws["dh1"], ws["dpre_a"])
                ops.gemm_tn(ws["dpre_a"], ws["h"], G(n0 + ".weight"), dbias=G(n0 + ".bias"))
                ops.gemm_nt(ws["dpre_a"], self._packed(ws, n0, dt, True), None, ws["dh"])
            else:
                ops.linear_small_bwd(ws["h1"], W[n3 + ".weight"], None, ws["dh2"], scratch(H), G(n3 + ".weight"), G(n3 + ".bias"),
                                     ws["dh1"], False)
                self._det_flush(ws["dh1"])
                ops.linear_small_bwd(ws["h"], W[n0 + ".weight"], ws["pre"][i], ws["dh1"], scratch(X), G(n0 + ".weight"), G(n0 + ".bias"),
                                     ws["dh"], False, OD_ACT_SILU)
                self._det_flush(ws["dh"])
            ops.rmsnorm_film_bwd(x[i], ws["inv1"][i], ssg, ws["dh"], dx, dssg, B, 1)        # dx += : the residual's gradient rides on
            self._linear_f32_bwd(ws, f"films.{i}", ws["c"], dssg, ws["dc"], accumulate_dx=i != a.depth - 1)
        if not f32:
            ops.cast_rows(dx, dxl)
        self._linear_f32_bwd(ws, "proj_in", ws["st"], dxl, None)
        if a.depth == 0:
            ws["dc"].zero_()
        self._det_flush(ws["dc"])
        ops.style_conditioning_bwd(ws["labels"], W["rff.W"].contiguous(), W["rff.b"], ws["dc"], G("cond_proj_w"), G("cond_proj_b"),
                                   G("null_labels"))
        self._det_flush(ar.grad)

    @torch.no_grad()
    def forward(self, st: torch.Tensor, labels: torch.Tensor):
        st = st.detach().float().contiguous()
        W = self._w()
        ssgs = self._films(self.compute_conditioning(labels), W)
        B = st.shape[0]
        u = torch.empty(B, dtype=torch.float32, device=st.device)
        v = torch.empty(B, self.style_dim, dtype=torch.float32, device=st.device)
        self._eval(st, ssgs, W, u, v)
        return u, v

    @torch.no_grad()
    def sample(self, labels: torch.Tensor, num_steps: int = 16, s_init: Optional[torch.Tensor] = None) -> torch.Tensor:
        B, dev = labels.shape[0], labels.device
        s = torch.randn(B, self.style_dim, device=dev) if s_init is None else s_init.detach().float().clone()
        W = self._w()
        ssgs = self._films(self.compute_conditioning(labels), W)          # label-only: once per call
        u, eta = self._b("smp.u", (B,), s), self._b("smp.eta", (2,), s)
        v = self._b("smp.v", (B, self.style_dim), s)
        x = self._b("smp.s", (B, self.style_dim, 1), s)
        x.copy_(s.view(B, self.style_dim, 1))
        xs = x.view(B, self.style_dim)
        self._eval(xs, ssgs, W, u, v)
        ops.sampler_eta(u, eta, self.c0, num_steps)

        def step():
            self._eval(xs, ssgs, W, u, v)
            ops.sampler_step(x, u, v.view(B, self.style_dim, 1), eta)

        if self.use_graph and dev.type == "cuda" and num_steps > 1:
            from .graph import CapturedLoop
            key = (B, dev, self._buf_gen, tuple(t.data_ptr() for t in W.values()))
            if getattr(self, "_graph", None) is None or self._graph[0] != key:
                if getattr(self, "_graph", None) is not None:
                    self._graph[1].close()
                self._graph = (key, CapturedLoop(step, dev))
            loop = self._graph[1]
            loop.begin()
            for _ in range(num_steps):
                loop.replay()
            loop.end()
        else:
            for _ in range(num_steps):
                step()
        return xs.clone()

    @torch.no_grad()
    def sample_many(self, labels_list: Sequence[torch.Tensor], num_steps: int = 16,
                    s_init: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
        """`sample` for G songs in one evaluation batch: labels_list[g] (B_g, 5) -> one (B_g, style_dim) per song.  The step size eta is
        computed per song over that song's rows (as its own `sample` computes it), and each song steps with its own.  Without `s_init`,
        the starting noise is drawn per song in song order: the draws G `sample` calls would make.  The loop is captured into one
        hipGraph per (rows, songs) shape; the song offsets are device data, not part of the graph's key."""
        G = len(labels_list)
        if G == 0 or (s_init is not None and len(s_init) != G):
            raise ValueError("sample_many needs one label batch per song (and one s_init per song when given)")
        dev, S = labels_list[0].device, self.style_dim
        Bs = [int(lab.shape[0]) for lab in labels_list]
        offs = [0]
        for n in Bs:
            offs.append(offs[-1] + n)
        B = offs[-1]
        inits = []
        for g in range(G):
            sg = torch.randn(Bs[g], S, device=dev) if s_init is None else s_init[g].detach().float()
            if tuple(sg.shape) != (Bs[g], S):
                raise ValueError(f"s_init[{g}] must be ({Bs[g]}, {S}), got {tuple(sg.shape)}")
            inits.append(sg)
        labels = torch.cat([lab.detach().float() for lab in labels_list], 0)
        W = self._w()
        ssgs = self._films(self.compute_conditioning(labels), W)          # label-only: once per call
        u, eta = self._b("smpm.u", (B,), labels), self._b("smpm.eta", (G, 2), labels)
        v = self._b("smpm.v", (B, S), labels)
        x = self._b("smpm.s", (B, S, 1), labels)
        offs_d = self._b("smpm.offs", (G + 1,), labels, torch.int32)
        lens_d = self._b("smpm.lens", (B,), labels, torch.int32)        # one frame per row
        host = torch.tensor(offs + [1] * B, dtype=torch.int32)
        if dev.type == "cuda":
            host = host.pin_memory()
        offs_d.copy_(host[:G + 1], non_blocking=True)
        lens_d.copy_(host[G + 1:], non_blocking=True)
        x.copy_(torch.cat(inits, 0).view(B, S, 1))
        xs = x.view(B, S)
        self._eval(xs, ssgs, W, u, v)
        ops.sampler_eta_groups(u, offs_d, eta, self.c0, num_steps)

        def step():
            self._eval(xs, ssgs, W, u, v)
            ops.sampler_step_varlen(x, u, v.view(B, S, 1), eta, lens_d, offs_d)

        if self.use_graph and dev.type == "cuda" and num_steps > 1:
            from .graph import CapturedLoop
            key = ("many", B, G, dev, self._buf_gen, tuple(t.data_ptr() for t in W.values()))
            if getattr(self, "_graph", None) is None or self._graph[0] != key:
                if getattr(self, "_graph", None) is not None:
                    self._graph[1].close()
                self._graph = (key, CapturedLoop(step, dev))
            loop = self._graph[1]
            loop.begin()
            for _ in range(num_steps):
                loop.replay()
            loop.end()
        else:
            for _ in range(num_steps):
                step()
        return [xs[offs[g]:offs[g + 1]].clone() for g in range(G)]
