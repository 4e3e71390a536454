"""The GEMM kernels at the shapes `LatentModel` launches them with, against fp64, tile by tile, through tests/test_gemm_paths.py's own runners,
input families and bounds (imported, not restated).  That file's table is the denoiser's (N >= 130, K >= one slab, M >= 33, outputs inside
wider buffers); the latent model (osu_dreamer_amd/latent.py, latent_grad.py) calls the same entry points with K below one k slab, N = 2,
ldc = N, M = 1 and accumulate at K = 8.

1. `latent_gemm_calls` is the list of GEMM calls one `LatentModel` forward (and backward) makes, as a pure function of the model's dimensions.
   `test_recorded_calls_match_the_shape_function` wraps ops.gemm_nt / ops.gemm_tn, runs the fixture models and compares the multisets.
2. `classify` reduces a call to its class: dispatch row (test_gemm_paths.nt_path / tn_path), K, N and M classes, ldc = N, accumulate, bias
   (TN: K a multiple of the 16-byte load chunk, lda > K, the block map, dbias).  `test_case_table_covers_every_class_of_the_model` evaluates the
   function for the tiny fixtures (emulator and GPU thresholds), `wide` and the shipped latent.yml (GPU thresholds) and fails with the list
   of classes no case of this file has.
3. The cases: the smallest shape of every class, on both backends; the model's real extremes (65 664 rows, M = 1, 2, 3) on the GPU.  Every
   class runs the integer family (exact: zero tolerance, element by element), the random family, cancel where K has two 16-byte chunks, in
   two layouts: `fenced` (test_gemm_paths' own: column offset 8, ld wider than the extent) and `model` (what the model passes: contiguous
   operands and output, lda = K and ldc = N exactly — TN: lda = hp > K with NaN in columns K..lda — each inside a buffer with 64 NaN
   elements either side).  Every launch runs twice: same bits (TN: in the deterministic mode and in the integer family, as in test_gemm_paths).
4. Bounds: test_gemm_paths.nt_bound / tn_bound per output tile (the kernel's own, clipped to the matrix) and over everything.  No case
   needed another bound (the worst narrow case sits at 0.56 of its imported bound on the MI355X, bf16 2 x 2 x 128, and at 0.62 on the
   emulator, bf16 1 x 2 x 16), so the fall-back rule of tests/test_step_paths.py (4 x torch's own error in the operand type, at least
   8 eps) is not used.
   The chained pair of latent_grad.py (dys = dsc x scores.T, then += dva x values.T) is compared with fp64 of the sum against
   |dsc| |Ws| + |dva| |Wv| under nt_bound(K_scores + K_values).

Each check prints `MEASURED <case> [<dispatch row>] <what> <backend> <worst tile error> <bound>` (test_gemm_paths.measured).
"""
import os
from collections import Counter
from dataclasses import dataclass, replace

import pytest
import torch

import test_gemm_paths as GP
from osu_dreamer_amd import _lib, ops
from osu_dreamer_amd.latent import LatentModel, LatentModelArgs, LayerArgs
from test_gemm_paths import BK, EMU_TH, GPU_TH, NT, TN, cdiv, nt_path, run_nt, run_tn, tn_path
from tools.gen_latent_grad_golden import CASES, grad_inputs, grad_weights, model_args, objective
from kernel_backend import REPO, dev  # noqa: F401

CH = {"bf16": 8, "fp32": 4, "x3": 4}                 # elements per 16-byte load chunk


# ---------------------------------------------------------------- 1. the calls a LatentModel makes
@dataclass(frozen=True)
class Call:
    """One GEMM launch.  nt: C[M, N] (+)= A[M, K] W[N, K]^T (+ bias); lda, ldw, ldc are the leading dimensions of A, W and C.
    tn: dW[N, K] += G[M, N]^T A[M, K]; lda is A's, ldw is G's and ldc is dW's (always K: ops.gemm_tn takes a contiguous dW)."""
    entry: str               # "nt" | "tn"
    T: str                   # bf16 | fp32 | x3
    M: int
    N: int
    K: int
    lda: int
    ldw: int
    ldc: int
    bias: bool = True        # nt: a bias is passed
    epi: str = "none"
    acc: bool = False
    n_block: int = 0         # tn: the block map (the padded SwiGLU width)
    n_valid: int = 0
    dbias: bool = False      # tn: dbias is passed


def latent_gemm_calls(h_dim, heads, hd, n_downs, stride, n_layers, expand, B, L, grad, T="fp32", Ba=None):
    """Every ops.gemm_nt / ops.gemm_tn call of `encode_chart(chart)`, `audio_encoder(audio)` and `decode_logits(z, s, skips)` on a chart of
    (B, 9, L) and a spectrogram of (Ba, 72, L) (Ba = B, or 1: one audio row for every chart), in the operand type T (fp32, bf16, or x3 =
    f32_matmul 'bf16x3', no-grad only); grad: the training forward and its backward as well (latent_grad.py).  Read from the call sites."""
    D, Ba = h_dim, B if Ba is None else Ba
    hf = int(D * expand * 2 / 3)
    hp = cdiv(hf, 64) * 64
    hpad = cdiv(heads, 8) * 8
    l = L // stride ** n_downs
    out = []

    def nt(M, N, K, bias=True, acc=False, T_=T, ldw=None):
        out.append(Call("nt", T_, M, N, K, K, K if ldw is None else ldw, N, bias, "none", acc))

    def tn(M, N, K, ldg, lda, T_=T, blk=0, valid=0):
        out.append(Call("tn", T_, M, N, K, lda, ldg, K, False, "none", False, blk, valid, True))

    def layer(M):
        for _ in range(n_layers):
            nt(M, 2 * hp, D)                                # proj_vg.1, row-mapped bias
            nt(M, D, hp)                                    # proj_o
            if grad:
                tn(M, D, hf, D, hp)                         # proj_o.weight: k_cols = hf, lda = hp
                nt(M, hp, D, bias=False)                    # dfo x proj_o.T
                tn(M, 2 * hp, D, 2 * hp, D, blk=hp, valid=hf)   # proj_vg.1.weight
                nt(M, D, 2 * hp, bias=False)                # dvg x proj_vg.1.T

    # encode_chart
    nt(B * L, D, 16)                                        # chart_encoder.0: 9 channels in one 16-wide chunk
    for i in range(n_downs):
        layer(B * L // stride ** i)
    layer(B * l)                                            # style_head.0
    nt(B * l, heads, D)                                     # scores -> sc (M, heads)
    nt(B * l, heads * hd, D)                                # values
    layer(B * l)                                            # temporal_layer
    if grad:
        tn(B * l, heads, D, hpad, D)                        # scores.weight: n_cols = heads of dsc's hpad columns
        tn(B * l, heads * hd, D, heads * hd, D)             # values.weight
        nt(B * l, D, hpad, bias=False)                      # dys = dsc x scores.T
        nt(B * l, D, heads * hd, bias=False, acc=True)      # dys += dva x values.T
        tn(B * L, D, 16, D, 16)                             # chart_encoder.0 (dw16)
    # audio_encoder: on the grad path SpecFeatures' projection stays fp32, on the parameter itself
    nt(Ba * L, D, 96, T_="fp32" if grad else T)
    for i in range(n_downs):
        layer(Ba * L // stride ** i)
    if grad:
        tn(Ba * L, D, 96, D, 96, T_="fp32")                 # net.8.weight
        nt(Ba * L, 96, D, bias=False, T_="fp32")            # dpre x w8t
    # decode_logits
    for i in range(n_downs):
        Lu = l * stride ** (i + 1)
        nt(Ba * Lu, D, D)                                   # mixer proj.0 on the skip
        nt(B * Lu, D, D)                                    # mixer gate
        layer(B * Lu)
        if grad:
            tn(Ba * Lu, D, D, D, D)                         # proj.0.weight
            nt(Ba * Lu, D, D, bias=False)                   # dp x proj.0.T
            tn(B * Lu, D, D, D, D)                          # gate.weight
            nt(B * Lu, D, D, bias=False, acc=True)          # dxm += dgx x gate.T
    return out


def calls_of_case(c, T, grad):
    return latent_gemm_calls(c.h_dim, c.heads, c.head_dim, c.n_downs, c.stride, c.n_layers, c.expand, c.B, c.L, grad, T, c.Ba)


# the inference fixtures of tests/test_latent.py (LATENT_TINY: h_dim 32, expand 4, 2 heads of 8; B, Ba, L) and its single-chunk edge shape, where
# the coarse levels have 1 and 2 rows
@dataclass(frozen=True)
class Infer:
    h_dim: int
    n_downs: int
    n_layers: int
    B: int
    Ba: int
    L: int
    expand: int = 4
    stride: int = 3
    heads: int = 2
    head_dim: int = 8


INFER = {"latent_tiny": Infer(32, 2, 2, 3, 1, 63), "latent_tiny_b2": Infer(32, 2, 2, 2, 2, 45), "one_chunk": Infer(32, 2, 2, 1, 1, 9),
         "one_chunk_b2": Infer(16, 2, 1, 2, 1, 9), "latent_full": Infer(128, 3, 8, 2, 1, 162, heads=2, head_dim=8)}
TINY_INFER = ("latent_tiny", "latent_tiny_b2", "one_chunk", "one_chunk_b2")
TINY_GRAD = tuple(n for n, c in CASES.items() if c.h_dim <= 64)
# latent.yml: h_dim 128, 16 heads of 64, n_downs 3, stride 3, 8 layers, expand 4, batch 32 of 2052 frames
YML = Infer(128, 3, 8, 32, 32, 2052, heads=16, head_dim=64)


def sources(which):
    """{source name: calls}: `emu` — what the tiny fixtures launch; `gpu` — those, `wide` / latent_full and latent.yml."""
    src = {}
    for n in TINY_INFER + (("latent_full",) if which == "gpu" else ()):
        src[n] = [c for T in ("fp32", "bf16", "x3") for c in calls_of_case(INFER[n], T, False)]
    for n in TINY_GRAD + (("wide",) if which == "gpu" else ()):
        src["grad_" + n] = [c for T in ("fp32", "bf16") for c in calls_of_case(CASES[n], T, True)]
        src["grad_" + n] += [c for T in ("fp32", "bf16", "x3") for c in calls_of_case(CASES[n], T, False)]
    if which == "gpu":
        src["latent.yml"] = [c for T in ("fp32", "bf16") for c in calls_of_case(YML, T, True)]
        src["latent.yml"] += [c for T in ("fp32", "bf16", "x3") for c in calls_of_case(YML, T, False)]
    return src


def test_latent_yml_is_the_configuration_evaluated():
    import yaml
    y = yaml.safe_load(open(os.path.join(REPO, "osu_dreamer_amd", "latent.yml")))
    m, a = y["model"], y["model"]["latent_args"]
    got = Infer(a["h_dim"], m["n_downs"], a["ae_args"]["n_layers"], y["data"]["batch_size"], y["data"]["batch_size"], y["data"]["seq_len"],
                a["ae_args"]["expand"], m["stride"], a["style_heads"], a["style_head_dim"])
    assert got == YML
    big = {(c.entry, c.T, c.M, c.N, c.K) for c in calls_of_case(YML, "bf16", True)}
    # the extremes the GPU cases below run
    assert {("nt", "bf16", 65664, 128, 16), ("nt", "bf16", 65664, 768, 128), ("nt", "bf16", 2432, 16, 128), ("tn", "bf16", 65664, 128, 341),
            ("tn", "bf16", 65664, 768, 128), ("nt", "fp32", 65664, 128, 96)} <= big


# ---------------------------------------------------------------- 2. classes
def k_class(K, slab):
    return "sub-slab" if K < slab else "slabs" if K % slab == 0 else "slabs+tail"


def n_class(N):
    return "N<8" if N < 8 else "N%8" if N % 8 else "N<128" if N < 128 else "N>=128"


def m_class(M, tile):
    return "M<tile" if M < tile else "exact" if M % tile == 0 else "ragged"


def classify(c, th):
    """(entry, dispatch row, K class, N class, M class, ldc = N, accumulate, bias) and for TN (K % chunk = 0, lda > K, block map, dbias).
    M is measured against the path's row tile (TN: the reduction slab, 64 bf16 / 32 fp32 rows), K against the k slab (TN: the 128-column
    output tile)."""
    if c.entry == "nt":
        p = nt_path(c.T, c.M, c.N, c.K, c.epi, c.acc, c.ldc, th=th)
        return ("nt", p.row, k_class(c.K, BK[c.T]), n_class(c.N), m_class(c.M, p.tile[0]), c.ldc == c.N, c.acc, c.bias)
    p = tn_path(c.T, c.M, c.N, c.K, th)
    return ("tn", p.row, k_class(c.K, 128), n_class(c.N), m_class(c.M, BK[c.T]), c.K % CH[c.T] == 0, c.lda > c.K, bool(c.n_block), c.dbias)


# ---------------------------------------------------------------- the recorder
def record(monkeypatch):
    """Wrap ops.gemm_nt / ops.gemm_tn (latent.py and latent_grad.py call them through the module): log the Call, then call through."""
    log = []
    real_nt, real_tn = ops.gemm_nt, ops.gemm_tn
    name = {torch.bfloat16: "bf16", torch.float32: "fp32"}

    def gemm_nt(A, W, bias, C, epilogue=ops.OD_EPI_NONE, accumulate=False, x3=False):
        assert not isinstance(W, ops.SplitWeight), "the latent model packs plain weights"
        T = "x3" if x3 and A.dtype == torch.float32 else name[A.dtype]
        log.append(Call("nt", T, A.shape[0], W.shape[0], A.shape[1], A.stride(0), W.stride(0), C.stride(0), bias is not None,
                        {ops.OD_EPI_NONE: "none", ops.OD_EPI_SILU: "silu"}[epilogue], bool(accumulate)))
        return real_nt(A, W, bias, C, epilogue=epilogue, accumulate=accumulate, x3=x3)

    def gemm_tn(G, A, dW, n_cols=None, k_cols=None, dbias=None, n_block=0, n_valid=0):
        N = n_cols if n_cols is not None else G.shape[1]
        K = k_cols if k_cols is not None else A.shape[1]
        log.append(Call("tn", name[G.dtype], G.shape[0], N, K, A.stride(0), G.stride(0), K, False, "none", False, n_block, n_valid,
                        dbias is not None))
        return real_tn(G, A, dW, n_cols=n_cols, k_cols=k_cols, dbias=dbias, n_block=n_block, n_valid=n_valid)

    monkeypatch.setattr(ops, "gemm_nt", gemm_nt)
    monkeypatch.setattr(ops, "gemm_tn", gemm_tn)
    return log


def diff(got, want):
    got, want = Counter(got), Counter(want)
    return {"recorded, not in the function": sorted((got - want).items(), key=str), "in the function, not recorded": sorted((want - got).items(), key=str)}


def infer_model(c, device):
    m = LatentModel(6, 32, c.n_downs, c.stride, LatentModelArgs(h_dim=c.h_dim, ae_args=LayerArgs(c.n_layers, c.expand, 2), style_head_dim=c.head_dim,
                                                                  style_heads=c.heads))
    g = torch.Generator().manual_seed(3)
    x = {"chart": torch.rand(c.B, 9, c.L, generator=g), "audio": torch.randn(c.Ba, 72, c.L, generator=g),
         "z": torch.randn(c.B, 6, c.L // c.stride ** c.n_downs, generator=g), "s": torch.randn(c.B, 32, generator=g)}
    return m.to(device), {k: v.to(device) for k, v in x.items()}


def check_infer_calls(name, device, monkeypatch):
    """encode_chart, audio_encoder and decode of a model with the fixture's dimensions (the launches do not depend on the weights), no-grad,
    in fp32, bf16 and bf16x3."""
    c = INFER[name]
    m, x = infer_model(c, device)
    log = record(monkeypatch)
    for T in ("fp32", "bf16", "x3"):
        m.compute_dtype = torch.bfloat16 if T == "bf16" else None
        m.f32_matmul = "bf16x3" if T == "x3" else "f32"
        del log[:]
        m.encode_chart(x["chart"])
        skips, _ = m.audio_encoder(x["audio"])
        m.decode(x["z"], x["s"], skips=skips)
        d = diff(log, calls_of_case(c, T, False))
        assert not any(d.values()), (name, T, d)


def grad_model(name, device, grad, bf16):
    c = CASES[name]
    a = model_args(c)
    m = LatentModel(a["emb_dim"], a["style_dim"], a["n_downs"], a["stride"], a["args"])
    m.load_state_dict(grad_weights(c))
    m = m.to(device)
    if bf16:
        m.compute_dtype = torch.bfloat16
    if grad:
        m.requires_grad_(True)
    return c, m, {k: v.to(device) for k, v in grad_inputs(c).items()}


def check_grad_calls(name, device, monkeypatch):
    """tests/test_latent_grad.py's objective and its backward in fp32 and bf16; the same objective with grad disabled in fp32, bf16 and bf16x3."""
    log = record(monkeypatch)
    for T in ("fp32", "bf16"):
        c, m, x = grad_model(name, device, True, T == "bf16")
        del log[:]
        objective(m, x).backward()
        d = diff(log, calls_of_case(c, T, True))
        assert not any(d.values()), (name, T, "grad", d)
    for T in ("fp32", "bf16", "x3"):
        c, m, x = grad_model(name, device, False, T == "bf16")
        m.f32_matmul = "bf16x3" if T == "x3" else "f32"
        del log[:]
        with torch.no_grad():
            objective(m, x)
        d = diff(log, calls_of_case(c, T, False))
        assert not any(d.values()), (name, T, "no-grad", d)


@pytest.mark.parametrize("name", TINY_INFER + tuple("grad_" + n for n in TINY_GRAD))
def test_recorded_calls_match_the_shape_function(dev, name, monkeypatch):
    if name.startswith("grad_"):
        check_grad_calls(name[5:], dev, monkeypatch)
    else:
        check_infer_calls(name, dev, monkeypatch)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    _lib._lib = None
    _lib.lib()
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["latent_full", "grad_wide"])
def test_recorded_calls_match_the_shape_function_wide(gpu, name, monkeypatch):
    if name.startswith("grad_"):
        check_grad_calls(name[5:], gpu, monkeypatch)
    else:
        check_infer_calls(name, gpu, monkeypatch)


# ---------------------------------------------------------------- 3. the cases
# NT: (T, M, N, K, variant) with variant b = bias, n = no bias (the backward's data GEMMs), a = accumulate without bias.  The smallest shape of
# every class: M = 1, 2, 3 below the row tile, one tile (32 fp32 at WMT 1, 64 at WMT 2) for `exact`, a tile and 8 rows for `ragged`; N = 2
# (the scores), 16 / 32 (one partial column tile), 128 (one whole tile), 256 (two); K = 8 (dsc), 16, 32 below the bf16 slab of 64 (fp32: 8, 16
# below 32), whole slabs, and 96 = one bf16 slab and a 32-element tail.  They run on both backends: under the emulator's thresholds and under
# the GPU's these shapes reach the 64-row (fp32: 32-row) kernels.
NT_SHAPES = [
    ("bf16", 1, 2, 16, "b"), ("bf16", 2, 2, 128, "b"), ("bf16", 3, 16, 8, "n"), ("bf16", 1, 16, 16, "a"), ("bf16", 2, 16, 16, "b"), ("bf16", 3, 16, 64, "b"),
    ("bf16", 1, 16, 96, "b"), ("bf16", 2, 16, 128, "n"), ("bf16", 3, 128, 16, "b"), ("bf16", 1, 128, 16, "n"), ("bf16", 2, 128, 128, "a"),
    ("bf16", 3, 128, 128, "b"), ("bf16", 1, 128, 128, "n"), ("bf16", 64, 16, 128, "b"), ("bf16", 64, 128, 16, "n"), ("bf16", 64, 128, 128, "a"),
    ("bf16", 64, 128, 128, "b"), ("bf16", 64, 128, 128, "n"), ("bf16", 72, 32, 16, "b"), ("bf16", 72, 32, 32, "a"), ("bf16", 72, 32, 32, "n"),
    ("bf16", 72, 32, 64, "b"), ("bf16", 72, 32, 96, "b"), ("bf16", 72, 32, 128, "n"), ("bf16", 72, 128, 16, "b"), ("bf16", 72, 128, 32, "b"),
    ("bf16", 72, 128, 96, "b"), ("bf16", 72, 128, 128, "a"), ("bf16", 72, 128, 128, "b"), ("bf16", 72, 128, 128, "n"),
    ("fp32", 1, 2, 16, "b"), ("fp32", 2, 2, 32, "b"), ("fp32", 3, 16, 8, "n"), ("fp32", 1, 16, 16, "a"), ("fp32", 2, 16, 16, "b"), ("fp32", 3, 16, 32, "b"),
    ("fp32", 1, 32, 32, "n"), ("fp32", 2, 128, 16, "b"), ("fp32", 3, 128, 16, "n"), ("fp32", 1, 128, 32, "b"), ("fp32", 2, 128, 128, "a"),
    ("fp32", 3, 128, 128, "n"), ("fp32", 32, 16, 128, "b"), ("fp32", 32, 128, 16, "n"), ("fp32", 32, 128, 128, "a"), ("fp32", 32, 128, 128, "b"),
    ("fp32", 32, 128, 128, "n"), ("fp32", 40, 16, 16, "a"), ("fp32", 40, 16, 16, "b"), ("fp32", 40, 16, 16, "n"), ("fp32", 40, 32, 32, "a"),
    ("fp32", 40, 32, 32, "b"), ("fp32", 40, 32, 32, "n"), ("fp32", 40, 128, 16, "b"), ("fp32", 40, 128, 32, "b"), ("fp32", 40, 128, 128, "a"),
    ("fp32", 40, 128, 128, "n"), ("fp32", 136, 256, 32, "b"),
    ("x3", 1, 2, 16, "b"), ("x3", 2, 2, 32, "b"), ("x3", 3, 16, 16, "b"), ("x3", 1, 16, 32, "b"), ("x3", 2, 128, 16, "b"), ("x3", 3, 128, 32, "b"),
    ("x3", 64, 16, 128, "b"), ("x3", 64, 128, 128, "b"), ("x3", 72, 32, 16, "b"), ("x3", 72, 32, 32, "b"), ("x3", 72, 128, 16, "b"), ("x3", 72, 128, 32, "b"),
    # the 128-row form (WMT 4) with a single column tile: from 6 x 128 rows on the emulator (the GPU runs these on its 64- / 32-row kernels)
    ("bf16", 776, 128, 16, "b"), ("bf16", 776, 128, 96, "b"), ("bf16", 768, 128, 128, "a"), ("fp32", 776, 128, 16, "b"), ("fp32", 768, 128, 128, "a"),
    ("x3", 776, 128, 16, "b"), ("x3", 768, 128, 96, "b"),
]
# The model's own extremes (latent.yml: 32 x 2052 = 65 664 frames at level 0, 32 x 76 = 2 432 at the coarsest): the 128-row form below one slab
# and with the 32-element tail, accumulate at 65 664 rows, the 256 x 256 kernels on N = 768 / 384 (the 4-wave kernel in bf16, the 8-wave one in
# fp32 and x3), the pool's heads with ldc = 16, its values' 1024-deep accumulate, fp32 on 64-row tiles (57 x 6 = 342 tiles < 512, 684 >= 600)
NT_SHAPES_GPU = [
    ("bf16", 65664, 128, 16, "b"), ("bf16", 65664, 128, 96, "b"), ("bf16", 65664, 128, 128, "a"), ("bf16", 65664, 128, 128, "b"), ("bf16", 65664, 128, 128, "n"),
    ("bf16", 65664, 768, 128, "b"), ("bf16", 65664, 384, 128, "n"), ("bf16", 2432, 16, 128, "b"), ("bf16", 2432, 128, 1024, "a"),
    ("fp32", 65664, 128, 16, "b"), ("fp32", 65664, 128, 96, "b"), ("fp32", 65664, 128, 128, "a"), ("fp32", 65664, 128, 128, "n"), ("fp32", 65664, 96, 128, "n"),
    ("fp32", 65664, 768, 128, "b"), ("fp32", 65664, 384, 128, "n"), ("fp32", 7296, 768, 128, "b"), ("fp32", 2432, 16, 128, "b"),
    ("x3", 65664, 128, 16, "b"), ("x3", 65664, 128, 96, "b"), ("x3", 65664, 768, 128, "b"),
]
# TN: (T, M, N, K, ldg, lda, n_block, n_valid), always with dbias.  N = 2 of dsc's 8 columns; K = 42 / 341 = hf with lda = hp = 64 / 384 (K not a
# multiple of the 16-byte chunk, dW rows unaligned); K = 32 of lda 64 (s4r1: hf = 32); the 64 / 32, 64 / 42 and 384 / 341 block maps; M = 1, 2, 3
# below the reduction slab (64 bf16 / 32 fp32 rows), one slab, one slab and 8 rows.
TN_SHAPES = [
    ("bf16", 1, 2, 16, 8, 16, 0, 0), ("bf16", 2, 16, 16, 16, 16, 0, 0), ("bf16", 3, 16, 32, 16, 64, 0, 0), ("bf16", 1, 16, 128, 16, 128, 0, 0),
    ("bf16", 2, 32, 42, 32, 64, 0, 0), ("bf16", 3, 128, 16, 128, 16, 64, 32), ("bf16", 1, 128, 128, 128, 128, 0, 0), ("bf16", 2, 128, 341, 128, 384, 0, 0),
    ("bf16", 3, 768, 128, 768, 128, 384, 341), ("bf16", 64, 16, 128, 16, 128, 0, 0), ("bf16", 64, 128, 128, 128, 128, 0, 0),
    ("bf16", 64, 128, 341, 128, 384, 0, 0), ("bf16", 64, 768, 128, 768, 128, 384, 341), ("bf16", 72, 32, 16, 32, 16, 0, 0), ("bf16", 72, 32, 42, 32, 64, 0, 0),
    ("bf16", 72, 128, 16, 128, 16, 0, 0), ("bf16", 72, 128, 32, 128, 32, 64, 42), ("bf16", 72, 128, 128, 128, 128, 0, 0), ("bf16", 72, 128, 341, 128, 384, 0, 0),
    ("bf16", 72, 768, 128, 768, 128, 384, 341),
    ("fp32", 1, 2, 16, 8, 16, 0, 0), ("fp32", 2, 16, 16, 16, 16, 0, 0), ("fp32", 3, 16, 32, 16, 64, 0, 0), ("fp32", 1, 16, 128, 16, 128, 0, 0),
    ("fp32", 2, 32, 42, 32, 64, 0, 0), ("fp32", 3, 128, 16, 128, 16, 64, 32), ("fp32", 1, 128, 128, 128, 128, 0, 0), ("fp32", 2, 128, 341, 128, 384, 0, 0),
    ("fp32", 3, 768, 128, 768, 128, 384, 341), ("fp32", 32, 16, 128, 16, 128, 0, 0), ("fp32", 32, 128, 128, 128, 128, 0, 0),
    ("fp32", 32, 128, 341, 128, 384, 0, 0), ("fp32", 32, 768, 128, 768, 128, 384, 341), ("fp32", 40, 16, 16, 16, 16, 0, 0), ("fp32", 40, 16, 32, 16, 64, 0, 0),
    ("fp32", 40, 32, 42, 32, 64, 0, 0), ("fp32", 40, 128, 16, 128, 16, 0, 0), ("fp32", 40, 128, 16, 128, 16, 64, 32), ("fp32", 40, 128, 128, 128, 128, 0, 0),
    ("fp32", 40, 128, 341, 128, 384, 0, 0), ("fp32", 40, 768, 128, 768, 128, 384, 341), ("fp32", 72, 2, 32, 8, 32, 0, 0), ("bf16", 72, 2, 32, 8, 32, 0, 0),
]
# latent.yml at 65 664 rows: one tile and six (<= 8: the 512-workgroup split); the 341 of 384 columns; the 384 / 341 block map; 16 columns
TN_SHAPES_GPU = [
    ("bf16", 65664, 128, 16, 128, 16, 0, 0), ("bf16", 65664, 128, 128, 128, 128, 0, 0), ("bf16", 65664, 128, 341, 128, 384, 0, 0),
    ("bf16", 65664, 768, 128, 768, 128, 384, 341), ("bf16", 2432, 16, 128, 16, 128, 0, 0),
    ("fp32", 65664, 128, 16, 128, 16, 0, 0), ("fp32", 65664, 128, 128, 128, 128, 0, 0), ("fp32", 65664, 128, 341, 128, 384, 0, 0),
    ("fp32", 65664, 768, 128, 768, 128, 384, 341), ("fp32", 2432, 16, 128, 16, 128, 0, 0),
]
LAYOUTS = ("fenced", "model")


def nt_call(s):
    T, M, N, K, v = s
    return Call("nt", T, M, N, K, K, K, N, v == "b", "none", v == "a")


def tn_call(s):
    T, M, N, K, ldg, lda, blk, valid = s
    return Call("tn", T, M, N, K, lda, ldg, K, False, "none", False, blk, valid, True)


def nt_families(T, K):
    """integer (exact) and random everywhere; cancel where K holds two 16-byte chunks (its two subspaces need K >= 2 anyway)."""
    return ("integer", "random") + (("cancel",) if K >= 2 * CH[T] else ())


def nt_cases(s, layout):
    T, M, N, K, v = s
    return [NT(T, M, N, K, "none", fam, acc=v == "a", bias=v == "b", seed=i, layout=layout) for i, fam in enumerate(nt_families(T, K))]


def tn_cases(s, layout):
    """integer and random, each with the deterministic shadow off and on (run_tn: two deterministic runs bit-identical)."""
    T, M, N, K, ldg, lda, blk, valid = s
    ld = (ldg, lda) if layout == "model" else (0, 0)
    return [TN(T, M, N, K, fam, on, blk, valid, True, *ld) for fam in ("integer", "random") for on in (False, True)]


def ids(s):
    return "-".join(str(x) for x in s)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", NT_SHAPES, ids=ids)
def test_gemm_nt_narrow(dev, shape, layout):
    for c in nt_cases(shape, layout):
        run_nt(c, dev, twice=True)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", TN_SHAPES, ids=ids)
def test_gemm_tn_narrow(dev, shape, layout):
    for c in tn_cases(shape, layout):
        run_tn(c, dev, twice=True)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", NT_SHAPES_GPU, ids=ids)
def test_gemm_nt_narrow_large(gpu, shape, layout):
    for c in nt_cases(shape, layout):
        run_nt(c, gpu, twice=True)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", TN_SHAPES_GPU, ids=ids)
def test_gemm_tn_narrow_large(gpu, shape, layout):
    for c in tn_cases(shape, layout):
        run_tn(c, gpu, twice=True)


# ---------------------------------------------------------------- od_gemm_nt and an unaligned ldc
@pytest.mark.parametrize("acc", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("M", [3, 72])
@pytest.mark.parametrize("N", [2, 16])
@pytest.mark.parametrize("T", ["bf16", "fp32"])
def test_gemm_nt_contiguous_output_of_2_and_16_columns(dev, T, N, M, acc):
    """ldc = N = 2 (a bf16 row is 4 bytes: no 16-byte store fits, the kernel stores element by element) and ldc = N = 16, the pool's sc and va
    buffers, in both output types, exact: every element written once, nothing either side of the contiguous output touched."""
    c = NT(T, M, N, 32, "none", "integer", acc=acc, bias=not acc, layout="model")
    assert c.ldc == N and (N % 8 == 0) == (N == 16)
    run_nt(c, dev, twice=True)
    run_nt(replace(c, fam="random"), dev, twice=True)


# ---------------------------------------------------------------- the chained pair of latent_grad.py (chart_bwd)
def run_chain(T, M, D, heads, hv, fam, device):
    """dys = dsc x scores.T (K = 8: the `heads` score columns in one zero-padded chunk, bias None), then dys += dva x values.T (accumulate):
    fp64 of the sum of both products, measured against |dsc| |Ws| + |dva| |Wv|; one buffer, written then added to, as the model does."""
    tt = GP.TORCH[T]
    A1, W1, _, _, _, _ = GP.make_nt_inputs(fam, M, D, 8, device, bias=False, seed=21)
    A2, W2, _, _, _, _ = GP.make_nt_inputs(fam, M, D, hv, device, bias=False, seed=22)
    A1[:, heads:] = 0                                   # dsc's padding columns; the packed scores.T has zeros there as well
    W1[:, heads:] = 0
    ops_ = [GP.flat_buffer(tuple(t.shape), tt, device, t.to(tt))[1] for t in (A1, W1, A2, W2)]
    a1, w1, a2, w2 = ops_
    ref = a1.double() @ w1.double().t() + a2.double() @ w2.double().t()
    scale = a1.double().abs() @ w1.double().abs().t() + a2.double().abs() @ w2.double().abs().t()

    def launch():
        buf, dys = GP.flat_buffer((M, D), tt, device)
        ops.gemm_nt(a1, w1, None, dys)
        ops.gemm_nt(a2, w2, None, dys, accumulate=True)
        return buf, dys
    buf, dys = launch()
    p = nt_path(T, M, D, hv, acc=True, ldc=D, th=GPU_TH if device.type == "cuda" else EMU_TH)
    case = f"chain-{T}-{fam}-{M}x{D}x(8+{hv}) [{p.row}]"
    GP.assert_flat_contract(case, buf, "dys")
    if fam == "integer":
        bad = dys.double() != ref
        assert not bool(bad.any()), f"{case}: {int(bad.sum())} elements differ from the exact sum, first {tuple(int(i) for i in bad.nonzero()[0])}"
        GP.measured(case, "dys (exact)", dys, 0.0, 0.0)
    else:
        GP.check_tiles(case, "dys against |dsc| |Ws| + |dva| |Wv|", dys.double(), ref, *p.tile, GP.nt_bound(T, 8 + hv, "bf16" if T == "bf16" else "fp32"),
                       scale=scale)
    buf2, _ = launch()
    assert torch.equal(GP.bits(buf2), GP.bits(buf)), f"{case}: two runs differ"


@pytest.mark.parametrize("fam", ["integer", "random", "cancel"])
@pytest.mark.parametrize("M,D,heads,hv", [(3, 16, 2, 16), (10, 32, 2, 16), (72, 32, 2, 16)])
@pytest.mark.parametrize("T", ["bf16", "fp32"])
def test_scores_then_values_accumulate_chain(dev, T, M, D, heads, hv, fam):
    run_chain(T, M, D, heads, hv, fam, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["integer", "random", "cancel"])
@pytest.mark.parametrize("T", ["bf16", "fp32"])
def test_scores_then_values_accumulate_chain_large(gpu, T, fam):
    run_chain(T, 2432, 128, 16, 1024, fam, gpu)                 # latent.yml: 32 x 76 rows, 16 heads of 64


# ---------------------------------------------------------------- coverage
def table_classes(th, gpu_sizes):
    nt = NT_SHAPES + (NT_SHAPES_GPU if gpu_sizes else [])
    tn = TN_SHAPES + (TN_SHAPES_GPU if gpu_sizes else [])
    return {classify(nt_call(s), th) for s in nt} | {classify(tn_call(s), th) for s in tn}


def test_case_table_covers_every_class_of_the_model():
    """Every class of every call of the tiny fixtures (emulator thresholds: the cases both backends run; GPU thresholds), of `wide` /
    latent_full and of latent.yml (GPU thresholds) has a case; the rows reached are rows test_gemm_paths.py's table already lists."""
    missing = []
    for which, th, have in (("emu", EMU_TH, table_classes(EMU_TH, False)), ("gpu", GPU_TH, table_classes(GPU_TH, True))):
        for src, calls in sources(which).items():
            for k in sorted({classify(c, th) for c in calls} - have, key=str):
                missing.append((which, src, k))
    assert not missing, "classes of the model's GEMM calls without a case:\n" + "\n".join(str(m) for m in missing)
    rows = {k[1] for th, g in ((EMU_TH, False), (GPU_TH, True)) for k in table_classes(th, g)}
    print("dispatch rows the narrow cases reach:", sorted(rows))
    assert rows <= set(GP.ROWS), sorted(rows - set(GP.ROWS))
    # the cases are the model's layout: ldc = N, and the TN ones carry the model's leading dimensions
    assert all(nt_call(s).ldc == s[2] for s in NT_SHAPES + NT_SHAPES_GPU)
    # M = 1, 2 and 3 on every entry point and type
    for T in ("bf16", "fp32", "x3"):
        assert {s[1] for s in NT_SHAPES if s[0] == T} >= {1, 2, 3}
    for T in ("bf16", "fp32"):
        assert {s[1] for s in TN_SHAPES if s[0] == T} >= {1, 2, 3}
    # the GPU list against the function: every large shape is one latent.yml launches (by type, extent, bias and accumulate)
    yml = {(c.entry, c.T, c.M, c.N, c.K, c.bias, c.acc, c.lda, c.ldw, c.n_block, c.n_valid) for T in ("fp32", "bf16", "x3")
           for g in (False, True) if not (g and T == "x3") for c in calls_of_case(YML, T, g)}
    for s in NT_SHAPES_GPU:
        c = nt_call(s)
        assert ("nt", c.T, c.M, c.N, c.K, c.bias, c.acc, c.lda, c.ldw, 0, 0) in yml, s
    for s in TN_SHAPES_GPU:
        c = tn_call(s)
        assert ("tn", c.T, c.M, c.N, c.K, False, False, c.lda, c.ldw, c.n_block, c.n_valid) in yml, s
