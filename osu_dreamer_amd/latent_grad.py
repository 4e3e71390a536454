"""Backpropagation through `LatentModel` on the HIP path: the backward of `audio_encoder`, `encode_chart`, `decode_logits` and the label
predictor, as `torch.autograd.Function`s over the kernels of csrc/latent.hip (reference autograd of
osu_dreamer/models/latent/{model,unet,spec_features}.py).

There is one forward, in latent.py: the Functions run it with a `_Tape` as its storage policy where inference runs it with `_Slots`.  The
tape hands out a fresh tensor per request, has the residual and the mixer write to a new tensor, and keeps what the backward reads (each
block's input, h, hd, vg, hh, inv_rms, fo and FiLM rows; the resampled streams; the heads' inputs) in tensors owned by that call, never in
the model's shape-keyed inference workspaces, so several forwards can be alive at once.  Parameters are inputs of the Functions, so
autograd fills their `.grad`; parameter gradients are fp32, activations and their gradients are of the compute dtype (fp32, or bf16 with
fp32 accumulation), except SpecFeatures (audio_encoder.0), which runs in fp32 in both.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import det, ops
from ._lib import OD_ACT_NONE, OD_ACT_SILU

F32 = torch.float32


class _Tape:
    def __init__(self, m, names: List[str]):
        self.m, self.names = m, names
        self.dt = m._dtype()
        self.pk = m._pack(self.dt, train=True)
        self.dev = m.P("proj_out.weight").device
        self.G: Dict[str, torch.Tensor] = {}
        self._arena: Optional[torch.Tensor] = None
        self._ws: Optional[torch.Tensor] = None
        self._spent = False
        # OD_DETERMINISTIC: the shared kernels that add with fp32 atomics (od_gemm_tn, od_dwconv_bwd, od_proj_in_bwd, od_linear_small_bwd's
        # dx) then add into integer shadows of the buffers registered here, folded in by flush() before the first reader
        self.det = det.context(self.dev)

    # ------------------------------------------------------------------ the forward's storage policy (latent.py's `_Slots` is the other)
    fp32_front = True                       # SpecFeatures up to its SiLU runs in fp32 on the parameter itself, cast_rows after it

    def buf(self, name: str, shape, dtype) -> torch.Tensor:
        return torch.empty(shape, dtype=dtype, device=self.dev)

    def zeros(self, name: str, shape, dtype) -> torch.Tensor:
        return torch.zeros(shape, dtype=dtype, device=self.dev)

    def over(self, x: torch.Tensor) -> torch.Tensor:
        """Where a kernel that may update x in place writes: the backward reads x, so elsewhere."""
        return torch.empty_like(x)

    def fork(self, name: str, x: torch.Tensor) -> torch.Tensor:
        return x                            # (no layer writes over its input here)

    def skip(self, i: int, sk: torch.Tensor, skf: torch.Tensor) -> torch.Tensor:
        """skf: skip i (sk) as frames.  A caller's tensor, not a training audio_encoder's, read in place: the backward reads it, so keep
        its values."""
        return skf.clone() if self.own_skip[i] and skf.data_ptr() == sk.data_ptr() else skf

    def record(self, **kept):
        self.__dict__.update(kept)

    # ------------------------------------------------------------------ the backward's storage
    def E(self, rows: int, cols: int, dtype=None) -> torch.Tensor:
        return torch.empty(rows, cols, dtype=dtype or self.dt, device=self.dev)

    def g(self, name: str) -> torch.Tensor:
        """The fp32 gradient of a parameter, zero until its first contribution (every kernel adds)."""
        t = self.G.get(name)
        if t is None:
            if self._arena is None:         # one buffer for all of this call's parameter gradients (one range of the deterministic table)
                self._off, n = {}, 0
                for k in self.names:
                    self._off[k] = n
                    n += (self.m.P(k).numel() + 7) // 8 * 8
                self._arena = self.atomic(torch.zeros(n, dtype=F32, device=self.dev))
            p = self.m.P(name)
            t = self.G[name] = self._arena[self._off[name]:self._off[name] + p.numel()].view(p.shape)
        return t

    def atomic(self, t: torch.Tensor) -> torch.Tensor:
        """A contiguous fp32 buffer that a kernel with atomics adds into."""
        if self.det is not None:
            self.det.register(t)
        return t

    def flush(self, t: torch.Tensor) -> torch.Tensor:
        if self.det is not None:
            self.det.flush(t)
        return t

    def ws(self, n: int) -> torch.Tensor:
        """Scratch for the partial rows of one backward kernel (calls on one stream run in order, so they share it)."""
        if self._ws is None or self._ws.numel() < n:
            self._ws = torch.empty(n, dtype=F32, device=self.dev)
        return self._ws

    def begin_bwd(self):
        """Every kernel adds into this call's gradient buffers, which `.grad` may alias after the first backward: a second one would count
        everything twice."""
        if self._spent:
            raise RuntimeError("LatentModel: this forward was already backpropagated; a second backward through the same graph "
                               "(retain_graph=True) is not supported, run the forward again")
        self._spent = True

    def grads(self):
        if self._arena is not None:
            self.flush(self._arena)
        return tuple(self.G.get(n) for n in self.names)

    def to_frames(self, t: torch.Tensor) -> torch.Tensor:
        """(B, C, L) gradient -> [B*L][C] of the compute dtype; free for the permuted views the backwards hand back."""
        B, C, L = t.shape
        return t.to(self.dt).permute(0, 2, 1).contiguous().reshape(B * L, C)

    def layer_bwd(self, rec, dout: torch.Tensor, dcond: Optional[torch.Tensor]) -> torch.Tensor:
        """dout: the gradient of the layer's output.  Returns the gradient of its input; dcond (B, cond_dim) fp32 += through the films."""
        m, pk, g = self.m, self.pk, self.g
        p, blocks, x_last, cond, B, L = rec
        M, D, hf, hp = B * L, m.a_dim, m.hf, m.hp
        k = 1 + 2 * m.args.ae_args.radius
        ws = self.ws(ops.latent_bwd_ws_floats("film", B, L, D))
        dx = self.E(M, D)
        ops.rmsnorm_affine_film_bwd(x_last, m.P(p + "out_norm.gamma"), None, dout, dx, g(p + "out_norm.gamma"), None, ws, B, L)
        for i in reversed(range(len(blocks))):
            x, ssg, h, hd, vg, hh, inv, fo = blocks[i]
            b = f"{p}blocks.{i}.0."
            dssg = None if ssg is None else torch.zeros(B, 3 * D, dtype=F32, device=self.dev)
            dfo, dhh, dvg, dhd, dh = self.E(M, D), self.E(M, hp), self.E(M, 2 * hp), self.E(M, D), self.E(M, D)
            ops.rmsnorm_affine_gate_residual_bwd(fo, m.P(f"{p}blocks.{i}.1.gamma"), ssg, dx, dfo, g(f"{p}blocks.{i}.1.gamma"), dssg, ws, B, L)
            ops.gemm_tn(dfo, hh, g(b + "proj_o.weight"), n_cols=D, k_cols=hf, dbias=g(b + "proj_o.bias"))
            ops.gemm_nt(dfo, pk[b + "proj_o.T"], None, dhh)
            ops.swiglu_rmsnorm_bwd(vg, inv, dhh, dvg, hf, hp)
            ops.gemm_tn(dvg, hd, g(b + "proj_vg.1.weight"), n_cols=2 * hp, k_cols=D, dbias=g(b + "proj_vg.1.bias"), n_block=hp, n_valid=hf)
            ops.gemm_nt(dvg, pk[b + "proj_vg.1.T"], None, dhd)
            ops.dwconv_bwd(h, m.P(b + "proj_vg.0.weight"), dhd, dh, g(b + "proj_vg.0.weight"), g(b + "proj_vg.0.bias"), B, L, k)
            # dx holds the residual's share already: the norm's share is added to it
            ops.rmsnorm_affine_film_bwd(x, m.P(f"{p}norms.{i}.gamma"), ssg, dh, dx, g(f"{p}norms.{i}.gamma"), dssg, ws, B, L,
                                        accumulate_dx=True)
            if ssg is not None:
                lp = torch.empty(B, 3 * D, dtype=F32, device=self.dev)
                ops.linear_small_bwd(cond, m.P(f"{p}films.{i}.weight"), None, dssg, lp, g(f"{p}films.{i}.weight"), g(f"{p}films.{i}.bias"),
                                     dcond, True)
        return dx

    def down_bwd(self, name: str, x: torch.Tensor, dy: torch.Tensor, B: int, Lo: int) -> torch.Tensor:
        m = self.m
        dx = self.E(B * Lo * m.stride, m.a_dim)
        ws = self.ws(ops.latent_bwd_ws_floats("down", B, Lo, m.a_dim, m.stride))
        ops.unet_down_bwd(x, m.P(name + ".weight"), dy, dx, self.g(name + ".weight"), self.g(name + ".bias"), ws, B, Lo, m.stride)
        return dx

    def audio_bwd(self, dskips, dh):
        m, pk, g = self.m, self.pk, self.g
        Ba, L, D, p = self.Ba, self.L, m.a_dim, "audio_encoder.0.net."
        dx = None if dh is None else self.to_frames(dh)
        for i in reversed(range(m.n_downs)):
            rec, skip, Lo = self.levels[i]
            d = None if dskips[i] is None else self.to_frames(dskips[i])
            if dx is not None:      # (the last down conv feeds only h: without a gradient for h it gets none)
                dd = self.down_bwd(f"audio_encoder.1.downs.{i}.0", skip, dx, Ba, Lo)
                if d is not None:
                    ops.add_rows(d, dd)
                d = dd
            dx = None if d is None else self.layer_bwd(rec, d, None)
        if dx is None:
            return
        if self.dt != F32:
            dxt, dx = dx, self.E(Ba * L, D, F32)
            ops.cast_rows(dxt, dx)
        dpre, df, w8t = self.E(Ba * L, D, F32), self.E(Ba * L, 96, F32), self.E(96, D, F32)
        ops.pack_weight(m.P(p + "8.weight"), w8t, transpose=True)
        ops.rmsnorm_affine_film_bwd(self.pre, m.P(p + "9.gamma"), None, dx, dpre, g(p + "9.gamma"), None,
                                    self.ws(ops.latent_bwd_ws_floats("film", Ba, L, D)), Ba, L, act=OD_ACT_SILU)
        ops.gemm_tn(dpre, self.f96, g(p + "8.weight"), dbias=g(p + "8.bias"))
        ops.gemm_nt(dpre, w8t, None, df)
        names = ("1.weight", "1.bias", "2.gamma", "4.weight", "4.bias", "5.gamma")
        ops.spec_features_conv_bwd(self.audio, *(m.P(p + k) for k in names), df, *(g(p + k) for k in names),
                                   self.ws(ops.latent_bwd_ws_floats("spec", Ba, L, 0)))

    def chart_bwd(self, dz, ds_out):
        m, pk, g = self.m, self.pk, self.g
        B, l, D = self.B, self.l, m.a_dim
        heads, hd = m.args.style_heads, m.args.style_head_dim
        ds = self.atomic(torch.zeros(B, m.style_dim, dtype=F32, device=self.dev))
        if ds_out is not None:
            ds.copy_(ds_out)
        dh = None
        if dz is not None:
            dyt = self.E(B * l, D)
            ops.chart_head_bwd(self.yt, m.P("temporal_head.0.weight").view(m.emb_dim, D), m.P("temporal_head.0.bias"),
                               dz.to(F32).contiguous(), dyt, g("temporal_head.0.weight").view(m.emb_dim, D), g("temporal_head.0.bias"),
                               self.ws(ops.latent_bwd_ws_floats("head", B, l, D, m.emb_dim)), B, l, rms=True)
            dh = self.layer_bwd(self.rec_t, dyt, ds)            # s also reaches z through the temporal layer's films
        # style head: rms_norm <- proj_out <- AttnPool <- scores / values <- layer
        ds_pre = torch.empty_like(ds)
        ops.rmsnorm_rows_bwd(self.s_pre, None, self.flush(ds), ds_pre, None, 1e-6)
        dpooled = self.atomic(torch.empty_like(self.pooled))
        ops.linear_small_bwd(self.pooled, m.P("style_head.1.proj_out.weight"), None, ds_pre, torch.empty_like(ds_pre),
                             g("style_head.1.proj_out.weight"), g("style_head.1.proj_out.bias"), dpooled, False)
        # the score gradients sit in a zero-padded 8-column block: the GEMMs read whole 16-byte chunks
        dsc, dva, dys = torch.zeros(B * l, (heads + 7) // 8 * 8, dtype=self.dt, device=self.dev), self.E(B * l, heads * hd), self.E(B * l, D)
        ops.attn_pool_bwd(self.sc, self.va, self.flush(dpooled), dsc, dva, B, l, heads, hd)
        ops.gemm_tn(dsc, self.ys, g("style_head.1.scores.weight"), n_cols=heads, dbias=g("style_head.1.scores.bias"))
        ops.gemm_tn(dva, self.ys, g("style_head.1.values.weight"), dbias=g("style_head.1.values.bias"))
        ops.gemm_nt(dsc, pk["style_head.1.scores.T"], None, dys)
        ops.gemm_nt(dva, pk["style_head.1.values.T"], None, dys, accumulate=True)
        dh2 = self.layer_bwd(self.rec_s, dys, None)
        if dh is not None:
            ops.add_rows(dh, dh2)
        dx = dh2
        for i in reversed(range(m.n_downs)):
            rec, y, Lo = self.levels[i]
            dx = self.layer_bwd(rec, self.down_bwd(f"chart_encoder.1.downs.{i}.0", y, dx, B, Lo), None)
        dw16 = self.atomic(torch.zeros(D, 16, dtype=F32, device=self.dev))     # the padded operand's 16 columns; the 9 live ones are the weight's
        ops.gemm_tn(dx, self.cf, dw16, dbias=g("chart_encoder.0.bias"))
        g("chart_encoder.0.weight").view(D, -1).copy_(self.flush(dw16)[:, :m.P("chart_encoder.0.weight").shape[1]])

    def decode_bwd(self, dlogits: torch.Tensor):
        """Returns (dz, ds, [dskip per skip in the caller's order])."""
        m, pk, g = self.m, self.pk, self.g
        B, D, L = self.B, m.a_dim, self.Lout
        N = m.P("proj_out.weight").shape[0]
        dx = self.E(B * L, D)
        ops.chart_head_bwd(self.x_out, m.P("proj_out.weight").view(N, D), m.P("proj_out.bias"), dlogits.to(F32).contiguous(), dx,
                           g("proj_out.weight").view(N, D), g("proj_out.bias"), self.ws(ops.latent_bwd_ws_floats("head", B, L, D, N)), B, L)
        ds = self.atomic(torch.zeros(B, m.style_dim, dtype=F32, device=self.dev))
        dskips: List[Optional[torch.Tensor]] = [None] * m.n_downs
        for i in reversed(range(m.n_downs)):
            x_in, xu, skf, pr, gx, bc, Bs, rec, Li = self.ups[i]
            Lu = Li * m.stride
            mx = f"decoder.mixers.{i}."
            dxm = self.layer_bwd(rec, dx, ds)
            dp, dgx = self.E(Bs * Lu, D, F32 if bc else self.dt), self.E(B * Lu, D)
            ops.unet_mixer_bwd(pr, bc, gx, m.P(mx + "proj.1.gamma"), dxm, dp, dgx, g(mx + "proj.1.gamma"),
                               self.ws(ops.latent_bwd_ws_floats("mixer", B, Lu, D, int(bc))), B, Lu)
            if dp.dtype != self.dt:                              # the batch sum is fp32: the GEMMs take it in the compute dtype
                dpt = self.E(Bs * Lu, D)
                ops.cast_rows(dp, dpt)
                dp = dpt
            ops.gemm_tn(dp, skf, g(mx + "proj.0.weight"), dbias=g(mx + "proj.0.bias"))
            dskf = self.E(Bs * Lu, D)
            ops.gemm_nt(dp, pk[mx + "proj.0.T"], None, dskf)
            dskips[m.n_downs - 1 - i] = dskf.view(Bs, Lu, D).permute(0, 2, 1)
            ops.gemm_tn(dgx, xu, g(mx + "gate.weight"), dbias=g(mx + "gate.bias"))
            ops.gemm_nt(dgx, pk[mx + "gate.T"], None, dxm, accumulate=True)          # dxm is also the gradient of xu (the residual)
            dx = self.E(B * Li, D)
            ops.unet_up_bwd(x_in, m.P(f"decoder.ups.{i}.1.weight"), dxm, dx, g(f"decoder.ups.{i}.1.weight"), g(f"decoder.ups.{i}.1.bias"),
                            self.ws(ops.latent_bwd_ws_floats("up", B, Lu, D, m.stride)), B, Li, m.stride)
        E = self.z.shape[1]
        ops.proj_in_bwd(self.z, dx, g("proj_emb.weight").view(D, E), g("proj_emb.bias"))
        dz = torch.empty_like(self.z)
        ops.proj_in_bwd_input(dx, m.P("proj_emb.weight").view(D, E), dz)
        return dz, self.flush(ds), dskips

    def labels_bwd(self, dout: torch.Tensor):
        m, g = self.m, self.g
        dout = dout.to(F32).contiguous()
        dhid, ds = self.atomic(torch.empty_like(self.hid)), self.atomic(torch.empty_like(self.s))
        ops.linear_small_bwd(self.hid, m.P("label_predictor.2.weight"), None, dout, torch.empty_like(dout), g("label_predictor.2.weight"),
                             g("label_predictor.2.bias"), dhid, False, OD_ACT_NONE)
        ops.linear_small_bwd(self.s, m.P("label_predictor.0.weight"), self.hid_pre, self.flush(dhid), torch.empty_like(dhid),
                             g("label_predictor.0.weight"), g("label_predictor.0.bias"), ds, False, OD_ACT_SILU)
        return self.flush(ds)


def _names(m, *prefixes):
    return [n for n, _ in m.named_parameters() if n.startswith(prefixes)]


class _AudioFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tape, audio, *params):
        ctx.tape = tape
        ctx.set_materialize_grads(False)
        skips, h = tape.m._audio_fwd(tape, audio)
        return (*skips, h)

    @staticmethod
    def backward(ctx, *grads):
        ctx.tape.begin_bwd()
        ctx.tape.audio_bwd(grads[:-1], grads[-1])
        return (None, None) + ctx.tape.grads()


class _ChartFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tape, chart, *params):
        ctx.tape = tape
        ctx.set_materialize_grads(False)
        return tape.m._chart_fwd(tape, chart)

    @staticmethod
    def backward(ctx, dz, ds):
        ctx.tape.begin_bwd()
        if dz is not None or ds is not None:
            ctx.tape.chart_bwd(dz, ds)
        return (None, None) + ctx.tape.grads()


class _DecodeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tape, n_skips, z, s, *rest):
        ctx.tape, ctx.n_skips, ctx.skip_dtypes = tape, n_skips, [t.dtype for t in rest[:n_skips]]
        ctx.set_materialize_grads(False)
        return tape.m._decode_fwd(tape, z, s, rest[:n_skips], 0)

    @staticmethod
    def backward(ctx, dlogits):
        ctx.tape.begin_bwd()
        if dlogits is None:
            return (None,) * (4 + ctx.n_skips) + ctx.tape.grads()
        dz, ds, dskips = ctx.tape.decode_bwd(dlogits)
        dskips = [d.to(dt) for d, dt in zip(dskips, ctx.skip_dtypes)]
        return (None, None, dz, ds, *dskips) + ctx.tape.grads()


class _LabelsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tape, s, *params):
        ctx.tape = tape
        return tape.m._label_predictor(s, tape)

    @staticmethod
    def backward(ctx, dout):
        ctx.tape.begin_bwd()
        ds = ctx.tape.labels_bwd(dout)
        return (None, ds) + ctx.tape.grads()


def _tape(m, *prefixes):
    if m._x3():
        raise NotImplementedError("f32_matmul = 'bf16x3' is an inference mode: gradients need 'f32' (or compute_dtype = torch.bfloat16)")
    names = _names(m, *prefixes)
    return _Tape(m, names), [m.P(n) for n in names]


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.to(F32).contiguous()


def audio_encoder(m, audio: torch.Tensor):
    tape, params = _tape(m, "audio_encoder.")
    out = _AudioFn.apply(tape, _f32c(audio.detach()), *params)
    return list(out[:-1]), out[-1]


def encode_chart(m, chart: torch.Tensor):
    tape, params = _tape(m, "chart_encoder.", "style_head.", "temporal_layer.", "temporal_head.")
    return _ChartFn.apply(tape, _f32c(chart.detach()), *params)


def decode_logits(m, z: torch.Tensor, s: torch.Tensor, skips) -> torch.Tensor:
    skips = list(skips)
    tape, params = _tape(m, "proj_emb.", "decoder.", "proj_out.")
    tape.own_skip = [not isinstance(getattr(sk.grad_fn, "tape", None), _Tape) for sk in skips]
    return _DecodeFn.apply(tape, len(skips), _f32c(z), _f32c(s), *skips, *params)


def label_predictor(m, s: torch.Tensor) -> torch.Tensor:
    tape, params = _tape(m, "label_predictor.")
    return _LabelsFn.apply(tape, _f32c(s), *params)
