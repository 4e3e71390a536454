"""Generate tests/golden/*_hd128_*.npz: the REFERENCE's denoiser with head_dim 128, run on the CPU by oracle/make_golden.py's own recorders.

    python tools/gen_hd128_golden.py [out_dir]          (OSU_DREAMER_REFERENCE points at the reference checkout)

The fixtures hold recorded outputs only (arrays): weights and batches are regenerated from the seed on both sides (store_weights=False,
store_full=False), as the full-width fixtures of oracle/make_golden.py are.  `CASES` is imported by tests/test_model_hd128.py, which never
imports the reference.
  tiny_hd128_b2_l130             forward, bf16 forward, sampler, loss, gradients, two optimizer + EMA steps (gen_model), 2 heads x 128, L = 130:
                                 three 64-key tiles with a ragged last one, and a ragged 64-query block
  train_bf16_tiny_hd128_b2_l130  the reference's bf16-autocast step beside its fp32 step on the same inputs (gen_train_bf16)
  full_hd128_d2_b2_l96           backbone 512 as 4 heads x 128, depth 2 (gen_model)
"""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import denoiser_oracle as O  # noqa: E402

TINY_HD128 = O.Dims(emb_dim=6, a_dim=32, style_dim=8, global_cond_dim=32, backbone_dim=64, n_heads=2, head_dim=128, depth=2, expand=2,
                    radius=1, u_head_dim=16)
FULL_HD128 = O.Dims(depth=2, n_heads=4, head_dim=128)

# name -> (recorder, dims, B, L, seed)
CASES = {
    "tiny_hd128_b2_l130": ("model", TINY_HD128, 2, 130, 2100),
    "train_bf16_tiny_hd128_b2_l130": ("train_bf16", TINY_HD128, 2, 130, 2200),
    "full_hd128_d2_b2_l96": ("model", FULL_HD128, 2, 96, 2300),
}


def main():
    from oracle import make_golden as G
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden")
    torch.manual_seed(0)
    torch.set_num_threads(8)
    G._install_shims()
    for name, (kind, d, B, L, seed) in CASES.items():
        if kind == "model":
            G.gen_model(out_dir, name, d, B=B, L=L, seed=seed, store_weights=False, with_bf16=True)
        else:
            G.gen_train_bf16(out_dir, name, d, B=B, L=L, seed=seed, store_full=False)


if __name__ == "__main__":
    main()
