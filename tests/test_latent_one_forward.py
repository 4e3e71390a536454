"""`LatentModel` has one forward launch sequence (osu_dreamer_amd/latent.py) under two storage policies: workspace slots with grad disabled,
a tape of fresh tensors with grad (latent_grad.py keeps only the backward).  What holds between the two, on the fixtures of
tools/gen_latent_grad_golden.py (`wide` on the GPU only, as in test_latent_grad.py):

  fp32   z, s, logits, labels of the objective and every skip and h of `audio_encoder` are torch.equal between a model with
         requires_grad_(True) and an identical model without: the same kernels on the same operands in the same order
  bf16   z, s, labels are torch.equal; logits and the skips are not compared, because with grad the SpecFeatures front end up to its SiLU
         stays fp32 (test_latent_grad.py's docstring says why) and the audio stream therefore differs by that front end's bf16 rounding
  storage   a forward and backward with grad creates no inference workspace; a forward without grad creates no tape and its outputs carry no
            graph
"""
import gc

import pytest
import torch

from osu_dreamer_amd import latent_grad
from tools.gen_latent_grad_golden import CASES, objective
from test_latent_grad import make
from kernel_backend import dev  # noqa: F401


def forward(m, x):
    objective(m, x, keep := {})
    keep["skips"], keep["h"] = m.audio_encoder(x["audio"])
    return keep


def tapes():
    gc.collect()
    return [o for o in gc.get_objects() if type(o) is latent_grad._Tape]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_the_grad_forward_is_the_nograd_forward(dev, name, mode):
    bf16 = mode == "bf16"
    c, mg, x = make(name, dev, bf16=bf16)
    _, m0, _ = make(name, dev, grad=False, bf16=bf16)
    a, b = forward(mg, x), forward(m0, x)
    for k in ("z", "s", "logits", "labels", "h"):
        assert a[k].requires_grad and not b[k].requires_grad, k
    for k in ("z", "s", "labels") + (() if bf16 else ("logits", "h")):
        assert torch.equal(a[k].detach(), b[k]), k
    assert len(a["skips"]) == len(b["skips"]) == c.n_downs
    if not bf16:
        for i, (sg, s0) in enumerate(zip(a["skips"], b["skips"])):
            assert sg.requires_grad and not s0.requires_grad and torch.equal(sg.detach(), s0), f"skip {i}"


@pytest.mark.parametrize("name", list(CASES))
def test_each_policy_keeps_to_its_own_storage(dev, name):
    _, mg, x = make(name, dev)
    objective(mg, x).backward()
    assert all(p.grad is not None for n, p in mg.named_parameters() if not n.startswith(f"audio_encoder.1.downs.{mg.n_downs - 1}."))
    assert mg._ws == {}, "the grad path took an inference workspace"
    _, m0, _ = make(name, dev, grad=False)
    del mg
    before = tapes()
    out = forward(m0, x)
    assert all(o in before for o in tapes()), "the no-grad forward made a tape"
    assert all(t.grad_fn is None for t in (out["z"], out["s"], out["logits"], out["labels"], out["h"], *out["skips"]))
    assert m0._ws, "the no-grad forward runs in the model's workspaces"
