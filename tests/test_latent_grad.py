"""Gradients through `LatentModel` on the HIP path against the reference's own autograd (tests/golden/latent_grad_*.npz, recorded by
tools/gen_latent_grad_golden.py from the reference's LatentModel in fp64, fp32 and under bf16 autocast).

Rules:
  forward on the grad path   z, s, logits, labels within 2e-5 relative L2 of the reference (test_latent.py's rule); with grad disabled the
                             outputs are torch.equal to a model that never had grad turned on
  gradients, fp32            every parameter within 1e-3 relative L2 of the reference's fp64 gradient (the reference's
                             own fp32 run is at most 8e-6 from it on these cases)
  gradients, bf16            every tensor within 3 x the reference's own bf16-autocast error on that tensor
  style_head.1.scores.bias   true gradient zero (softmax is shift-invariant): norm <= 1e-5 of the scores.weight gradient's in fp32,
                             <= 3 x the reference's recorded bf16 value in bf16
  the last audio down-conv   feeds only h, which the objective does not read: gradient None or exactly zero
  trajectory                 5 torch.optim.SGD steps: objective within 1e-4 relative at every step, final weights under
                             test_trajectory.py's rule (per tensor, RMS distance <= 1e-5 rms|w| + 1e-3 rms|w - w0| + 1e-7)
`wide` (h_dim 128, 16 heads of 64) runs on the GPU only, as latent_full does; its gradients are known by norm and sub-sample, and both
sides' errors are taken by the generator's `sub_err`.

Tightest tensor: `wide` in bf16, `audio_encoder.0.net.2.gamma` (8 elements; limit 1.27e-2 = 3 x the reference's 4.23e-3, a tensor on which the
reference's own bf16 error is 2.5 x smaller than on its neighbours).  It is a sum over every frame of terms that went through SpecFeatures,
where a bf16-rounded operand's error does not average out; that is why the grad path keeps SpecFeatures up to its SiLU in fp32 in both
modes.  The test prints every tensor's error and limit.
"""
import os

import numpy as np
import pytest
import torch

from osu_dreamer_amd.latent import LatentModel
from tools.gen_latent_grad_golden import CASES, DEAD, TRAJ_LR, TRAJ_STEPS, ZERO_TRUE, grad_inputs, grad_weights, model_args, objective, sub_err
from kernel_backend import dev, rel_l2  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SCORES_W = "style_head.1.scores.weight"


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def make(name, device, grad=True, bf16=False):
    c = CASES[name]
    if device.type == "cpu" and c.h_dim > 64:
        pytest.skip("the full-width latent model runs on the GPU only")
    a = model_args(c)
    m = LatentModel(a["emb_dim"], a["style_dim"], a["n_downs"], a["stride"], a["args"])
    m.load_state_dict(grad_weights(c))
    m = m.to(device)
    if bf16:
        m.compute_dtype = torch.bfloat16
    if grad:
        m.requires_grad_(True)
    return c, m, {k: v.to(device) for k, v in grad_inputs(c).items()}


def run(name, device, bf16=False):
    c, m, x = make(name, device, bf16=bf16)
    keep = {}
    obj = objective(m, x, keep)
    obj.backward()
    return c, m, x, obj, keep


@pytest.mark.parametrize("name", list(CASES))
def test_forward_on_the_grad_path(dev, name):
    c, m, x, obj, keep = run(name, dev)
    fx = load("latent_grad_" + name)
    for k in ("z", "s", "logits", "labels"):
        assert tuple(keep[k].shape) == tuple(fx[k].shape) and rel_l2(keep[k], fx[k]) < 2e-5, (k, rel_l2(keep[k], fx[k]))
    assert float(obj.detach()) == pytest.approx(float(fx["obj"]), rel=2e-5, abs=2e-5 * float(fx["logits"].norm()))
    # grad disabled: today's path, bit for bit what a model that never had grad turned on returns
    _, m0, _ = make(name, dev, grad=False)
    with torch.no_grad():
        got, want = objective(m, x, a := {}), objective(m0, x, b := {})
    assert all(not a[k].requires_grad and torch.equal(a[k], b[k]) for k in a) and torch.equal(got, want)
    # ... and with grad enabled on a model whose parameters do not require grad
    z0, s0 = m0.encode_chart(x["chart"])
    assert not z0.requires_grad and torch.equal(z0, b["z"]) and torch.equal(s0, b["s"])


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_gradients_vs_reference(dev, name, mode):
    c, m, x, obj, keep = run(name, dev, bf16=mode == "bf16")
    fx = load("latent_grad_" + name)
    dead = DEAD.format(c.n_downs - 1)
    grads = {k: p.grad for k, p in m.named_parameters()}
    worst = ("", 0.0)
    for k, g in grads.items():
        if k.startswith(dead):
            assert g is None or not bool(g.any()), f"{k}: the conv that feeds only h got a gradient"
            continue
        assert g is not None and g.dtype == torch.float32 and bool(torch.isfinite(g).all()), k
        if k == ZERO_TRUE:
            lim = 1e-5 * float(grads[SCORES_W].norm()) if mode == "fp32" else 3 * float(fx["errbf." + k])
            assert float(g.norm()) <= lim, (k, float(g.norm()), lim)
            continue
        if c.full:
            err = rel_l2(g, fx["g64." + k])
        else:       # norm and a 512-element sub-sample
            err = sub_err(g.cpu(), fx["s64." + k], fx["n64." + k])
        lim = 1e-3 if mode == "fp32" else 3 * float(fx["errbf." + k])
        print(f"{name} {mode} {k}: {err:.3e} (limit {lim:.3e})")
        assert err <= lim, (k, err, lim)
        worst = max(worst, (k, err / lim), key=lambda t: t[1])
    print(f"[{name}/{mode}] worst {worst[0]} at {worst[1]:.3f} of its limit")


@pytest.mark.parametrize("name", ["tiny", "tiny_bcast"])
def test_decode_logits_input_gradients(dev, name):
    """d <decode_logits(z, s, skips), R1> / d (z, s, skips); with one audio row the skip gradient is the sum over the decoder rows."""
    c, m, x = make(name, dev)
    fx = load("latent_grad_" + name)
    skips, _ = m.audio_encoder(x["audio"])
    zin, sin = fx["z"].to(dev).clone().requires_grad_(True), fx["s"].to(dev).clone().requires_grad_(True)
    sk = [t.detach().clone().requires_grad_(True) for t in skips]
    (m.decode_logits(zin, sin, skips=list(sk)) * x["R1"]).sum().backward()
    assert rel_l2(zin.grad, fx["dec.dz"]) < 1e-3 and rel_l2(sin.grad, fx["dec.ds"]) < 1e-3
    for i, t in enumerate(sk):
        assert tuple(t.grad.shape) == tuple(fx[f"dec.dskip{i}"].shape) == (c.Ba, c.h_dim, t.shape[2])
        assert rel_l2(t.grad, fx[f"dec.dskip{i}"]) < 1e-3, i
    # inputs alone turn the grad path on: parameters that do not require grad get none
    _, m0, _ = make(name, dev, grad=False)
    z2 = fx["z"].to(dev).clone().requires_grad_(True)
    (m0.decode_logits(z2, fx["s"].to(dev), skips=[t.detach() for t in skips]) * x["R1"]).sum().backward()
    assert rel_l2(z2.grad, fx["dec.dz"]) < 1e-3 and all(p.grad is None for p in m0.parameters())


def test_two_training_forwards_alive_at_once(dev):
    """encode_chart twice before either backward: each backward sees its own activations and equals its solo run bit for bit.  Run in the
    deterministic mode (det.force): the GEMM, conv and linear backwards this path shares with the denoiser add with fp32 atomics otherwise,
    and then not even two solo runs agree in the last bits on the GPU."""
    from osu_dreamer_amd import det
    det.force(True)
    try:
        _two_forwards(dev)
    finally:
        det.force(None)


def _two_forwards(dev):
    c, m, x = make("tiny", dev)
    g = torch.Generator().manual_seed(5)
    charts = [x["chart"], torch.rand(x["chart"].shape, generator=g).to(dev)]
    R = torch.randn(c.B, c.emb, c.L // c.stride ** c.n_downs, generator=g).to(dev)

    def grads_of(fn):
        m.zero_grad(set_to_none=True)
        fn()
        return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    def loss(out):
        return (out[0] * R).sum() + (out[1] * x["R3"]).sum()
    solo = [grads_of(lambda ch=ch: loss(m.encode_chart(ch)).backward()) for ch in charts]
    for first in (0, 1):
        def both():
            outs = [m.encode_chart(ch) for ch in charts]
            m.zero_grad(set_to_none=True)
            loss(outs[first]).backward()
        got = grads_of(both)
        assert got.keys() == solo[first].keys()
        assert all(torch.equal(got[k], solo[first][k]) for k in got), [k for k in got if not torch.equal(got[k], solo[first][k])][:3]


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.full])
def test_sgd_trajectory(dev, name):
    """torch.optim.SGD edits the parameters in place and never calls invalidate(): packed GEMM operands that went stale would show here."""
    c, m, x = make(name, dev)
    fx = load("latent_grad_traj_" + name)
    w0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    opt = torch.optim.SGD(m.parameters(), lr=TRAJ_LR)
    for i in range(TRAJ_STEPS):
        opt.zero_grad(set_to_none=True)
        obj = objective(m, x)
        obj.backward()
        opt.step()
        print(f"{name} step {i}: objective {float(obj.detach()):.7g} (reference {float(fx['obj'][i]):.7g})")
        assert float(obj.detach()) == pytest.approx(float(fx["obj"][i]), rel=1e-4), i
    for k, w in m.state_dict().items():
        ref, n = fx["w." + k], max(1.0, float(w.numel())) ** 0.5
        tol = 1e-5 * float(ref.norm()) / n + 1e-3 * float((ref - w0[k].cpu()).norm()) / n + 1e-7
        err = float((w.detach().cpu() - ref).norm()) / n
        assert err <= tol, (k, err, tol)


def test_unsupported_with_grad_raises(dev):
    c, m, x = make("tiny", dev)
    Ls = [c.L] * c.B
    with pytest.raises(NotImplementedError, match="varlen"):
        m.encode_chart(x["chart"], lengths=Ls)
    with pytest.raises(NotImplementedError, match="varlen"):
        m.audio_encoder(x["audio"], lengths=Ls)
    z, s = m.encode_chart(x["chart"])
    with pytest.raises(NotImplementedError, match="varlen"):
        m.decode_logits(z, s, audio=x["audio"], lengths=Ls)
    m.f32_matmul = "bf16x3"
    with pytest.raises(NotImplementedError, match="bf16x3"):
        m.encode_chart(x["chart"])
    with pytest.raises(NotImplementedError, match="bf16x3"):
        m(x["audio"], z.detach(), s.detach())
    # both stay available without grad
    with torch.no_grad():
        m.encode_chart(x["chart"], lengths=Ls)
        m.encode_chart(x["chart"])


def test_second_backward_raises(dev):
    """The parameter gradients of a call are sums the kernels add into: a second backward through the same forward would count them twice."""
    c, m, x = make("tiny", dev)
    z, s = m.encode_chart(x["chart"])
    loss = (s * x["R3"]).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="already backpropagated"):
        loss.backward()


def test_skips_of_a_no_grad_call_are_kept(dev):
    """decode_logits on skips from a no-grad audio_encoder call: what happens to them (or to the model's inference workspaces) between
    the forward and the backward does not reach the gradients."""
    from osu_dreamer_amd import det
    c, m, x = make("tiny", dev)
    fx = load("latent_grad_tiny")
    z, s = fx["z"].to(dev), fx["s"].to(dev)

    def grads(disturb):
        m.zero_grad(set_to_none=True)
        with torch.no_grad():
            skips, _ = m.audio_encoder(x["audio"])
        out = m.decode_logits(z, s, skips=skips)
        if disturb:
            with torch.no_grad():
                m.audio_encoder(torch.flip(x["audio"], (2,)))
                for t in skips:
                    t.zero_()
        (out * x["R1"]).sum().backward()
        return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    det.force(True)
    try:
        a, b = grads(False), grads(True)
    finally:
        det.force(None)
    assert a.keys() == b.keys() and "decoder.mixers.0.proj.0.weight" in a
    assert all(torch.equal(a[k], b[k]) for k in a), [k for k in a if not torch.equal(a[k], b[k])][:3]
