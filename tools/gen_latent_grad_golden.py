"""Generate tests/golden/latent_grad_*.npz by running the REFERENCE's own LatentModel (osu_dreamer/models/latent/model.py) forward and
backward on the CPU.

    python tools/gen_latent_grad_golden.py [out_dir]          (OSU_DREAMER_REFERENCE points at the reference checkout)

The fixtures hold inputs' seeds, the pinned cotangents' seeds and recorded results only.  Weights are rebuilt from a seed on both sides by
`grad_weights` (the tests import it, and `CASES`, `grad_inputs`, `objective`; they never import the reference): this package's
constructor draws the reference's default conv / linear init, every zero-initialised tensor (the films, the mixer gates) is overwritten
with N(0, 0.1^2) and every gamma multiplied by 1 + 0.2 N(0, 1), so that no gradient is identically zero except the last audio down-conv's
(it feeds only h, which the objective does not read).  The reference model takes them with load_state_dict(strict=True).

The objective runs every path of the reference trainer's forward (models/latent/train.py) without its losses:
    z, s = encode_chart(chart);  logits, labels = model(audio, z + 0.2 noise, s swapped within pairs)
    obj = <logits, R1> + <labels, R2> + <s, R3>
Each file stores z, s, logits, labels, obj and every parameter gradient of the fp64 run (whole, as fp32, or for `wide` its norm and a
512-element sub-sample), and per tensor the norm of the reference's OWN fp32 and bf16-autocast gradients and their relative L2 error
against the fp64 one (for `wide`: `sub_err`, the measure the test applies to it; the gradients of those two runs themselves would put a
file past 1 MiB).  `tiny` and `tiny_bcast` also store the gradients of <decode_logits(z, s, skips), R1> with respect to z, s
and the skips; each tiny case has a second file with a 5-step torch.optim.SGD(lr = 1e-2) trajectory in fp32: the objective at every step
and the final weights.
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SUB = 512
TRAJ_STEPS, TRAJ_LR = 5, 1e-2
DEAD = "audio_encoder.1.downs.{}.0."            # .format(n_downs - 1): no gradient when h takes no part in the objective
ZERO_TRUE = "style_head.1.scores.bias"          # softmax is shift-invariant: the true gradient is zero


@dataclass(frozen=True)
class Case:
    emb: int
    style: int
    n_downs: int
    stride: int
    h_dim: int
    n_layers: int
    expand: int
    radius: int
    head_dim: int
    heads: int
    B: int
    L: int
    Ba: int
    seed: int
    full: bool = True          # whole gradients and a trajectory (False: norms and sub-samples)


CASES = {
    "tiny": Case(8, 16, 2, 3, 32, 2, 2, 2, 8, 2, 4, 36, 4, 1100),
    "tiny_bcast": Case(8, 16, 2, 3, 32, 2, 2, 2, 8, 2, 4, 36, 1, 1200),
    "s4r1": Case(6, 16, 1, 4, 16, 1, 3, 1, 8, 2, 2, 20, 2, 1300),          # stride 4: 5 taps; radius 1
    "wide": Case(6, 32, 3, 3, 128, 2, 4, 2, 64, 16, 2, 54, 2, 1400, full=False),
}


def model_args(c: Case):
    return dict(emb_dim=c.emb, style_dim=c.style, n_downs=c.n_downs, stride=c.stride,
                args=dict(h_dim=c.h_dim, ae_args=dict(n_layers=c.n_layers, expand=c.expand, radius=c.radius),
                          style_head_dim=c.head_dim, style_heads=c.heads))


def grad_weights(c: Case):
    """The case's state dict (fp32), from its seed."""
    from osu_dreamer_amd.latent import LatentModel
    a = model_args(c)
    state = torch.random.get_rng_state()
    try:
        torch.manual_seed(c.seed)
        sd = {k: v.detach().clone() for k, v in LatentModel(a["emb_dim"], a["style_dim"], a["n_downs"], a["stride"], a["args"]).state_dict().items()}
    finally:
        torch.random.set_rng_state(state)
    g = torch.Generator().manual_seed(c.seed + 1)
    for k in sd:
        if float(sd[k].abs().max()) == 0.0:
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
        if k.endswith("gamma"):
            sd[k] = sd[k] * (1 + 0.2 * torch.randn(sd[k].shape, generator=g))
    return sd


def grad_inputs(c: Case):
    g = torch.Generator().manual_seed(c.seed + 2)
    l = c.L // c.stride ** c.n_downs
    return {"chart": torch.rand(c.B, 9, c.L, generator=g), "audio": torch.randn(c.Ba, 72, c.L, generator=g),
            "noise": torch.randn(c.B, c.emb, l, generator=g), "R1": torch.randn(c.B, 9, c.L, generator=g),
            "R2": torch.randn(c.B, 5, generator=g), "R3": torch.randn(c.B, c.style, generator=g),
            "perm": torch.arange(c.B) ^ 1}


def objective(model, x, keep=None):
    """The scalar above on any LatentModel-like `model`; x: grad_inputs moved to the model's device (and dtype for the fp64 run)."""
    z, s = model.encode_chart(x["chart"])
    logits, labels = model(x["audio"], z + 0.2 * x["noise"].to(z.dtype), s[x["perm"]])
    if keep is not None:
        keep.update(z=z, s=s, logits=logits, labels=labels)
    return (logits * x["R1"].to(logits.dtype)).sum() + (labels * x["R2"].to(labels.dtype)).sum() + (s * x["R3"].to(s.dtype)).sum()


def sub(t: torch.Tensor, n: int = SUB) -> torch.Tensor:
    t = t.detach().flatten()
    return t[::max(1, t.numel() // n)][:n]


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def sub_err(g, s_ref, n_ref):
    """The distance of a gradient from a reference known by its sub-sample and norm (`wide`): the larger of the sub-sample's relative L2
    error and the norm's relative error.  The reference's own fp32 and bf16 errors of such a case are recorded by this same measure."""
    return max(rel(sub(g), s_ref), abs(float(g.double().norm()) - float(n_ref)) / float(n_ref))


def _reference(c: Case, dtype):
    from osu_dreamer.models.latent.model import LatentModel, LatentModelArgs
    from osu_dreamer.models.latent.unet import LayerArgs
    a = model_args(c)
    aa = a["args"]
    m = LatentModel(a["emb_dim"], a["style_dim"], a["n_downs"], a["stride"],
                    LatentModelArgs(h_dim=aa["h_dim"], ae_args=LayerArgs(**aa["ae_args"]), style_head_dim=aa["style_head_dim"],
                                    style_heads=aa["style_heads"]))
    m.load_state_dict(grad_weights(c), strict=True)
    return m.to(dtype)


def _cast(x, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in x.items()}


def _run(c: Case, dtype, autocast=False):
    m = _reference(c, dtype)
    x, keep = _cast(grad_inputs(c), dtype), {}
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        obj = objective(m, x, keep)
    obj.backward()
    return m, obj, keep, {k: p.grad for k, p in m.named_parameters()}


def gen_case(out_dir, name, c: Case):
    m64, obj, keep, g64 = _run(c, torch.float64)
    _, _, _, g32 = _run(c, torch.float32)
    _, _, _, gbf = _run(c, torch.float32, autocast=True)
    dead = DEAD.format(c.n_downs - 1)
    fx = {"obj": np.float64(float(obj))}
    fx.update({k: v.detach().to(torch.float32).numpy() for k, v in keep.items()})
    worst32 = 0.0
    for k, g in g64.items():
        if k.startswith(dead):
            assert g is None and g32[k] is None and gbf[k] is None, k
            continue
        assert float(g.norm()) > 0 or k == ZERO_TRUE, k
        fx["n64." + k] = np.float64(float(g.norm()))
        if c.full:
            fx["g64." + k] = g.to(torch.float32).numpy()
        else:
            fx["s64." + k] = sub(g).to(torch.float32).numpy()
        for tag, gg in (("32", g32), ("bf", gbf)):
            fx[f"n{tag}." + k] = np.float64(float(gg[k].norm()))
            err = float(gg[k].norm()) if k == ZERO_TRUE else rel(gg[k], g) if c.full else sub_err(gg[k], sub(g), g.norm())
            fx[f"err{tag}." + k] = np.float64(err)
        if k != ZERO_TRUE:
            worst32 = max(worst32, float(fx["err32." + k]))
    if c.full and c.n_downs == 2:
        # decode_logits alone: gradients with respect to z, s and the skips (one audio row: the sum over the decoder rows)
        x = _cast(grad_inputs(c), torch.float64)
        skips, _ = m64.audio_encoder(x["audio"])
        zin = keep["z"].detach().clone().requires_grad_(True)
        sin = keep["s"].detach().clone().requires_grad_(True)
        sk = [t.detach().clone().requires_grad_(True) for t in skips]
        (m64.decode_logits(zin, sin, skips=list(sk)) * x["R1"]).sum().backward()
        fx["dec.dz"], fx["dec.ds"] = zin.grad.to(torch.float32).numpy(), sin.grad.to(torch.float32).numpy()
        for i, t in enumerate(sk):
            fx[f"dec.dskip{i}"] = t.grad.to(torch.float32).numpy()
    np.savez_compressed(os.path.join(out_dir, f"latent_grad_{name}.npz"), **fx)
    print(f"{name}: obj {float(obj):.6f}, {len(g64)} tensors, reference fp32 vs fp64 worst {worst32:.2e}, "
          f"scores.bias fp32 {float(fx['err32.' + ZERO_TRUE]) / float(fx['n32.style_head.1.scores.weight']):.1e} of scores.weight")
    if c.full:
        gen_traj(out_dir, name, c)


def gen_traj(out_dir, name, c: Case):
    m = _reference(c, torch.float32)
    x = grad_inputs(c)
    opt = torch.optim.SGD(m.parameters(), lr=TRAJ_LR)
    objs = []
    for _ in range(TRAJ_STEPS):
        opt.zero_grad(set_to_none=True)
        obj = objective(m, x)
        obj.backward()
        opt.step()
        objs.append(float(obj))
    fx = {"obj": np.asarray(objs, dtype=np.float64)}
    fx.update({"w." + k: v.detach().numpy() for k, v in m.state_dict().items()})
    np.savez_compressed(os.path.join(out_dir, f"latent_grad_traj_{name}.npz"), **fx)
    print(f"{name}: trajectory objectives {objs}")


def main():
    from oracle.make_golden import _install_shims
    _install_shims()
    torch.set_float32_matmul_precision("highest")
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden")
    for name, c in CASES.items():
        gen_case(out_dir, name, c)


if __name__ == "__main__":
    main()
