"""od_loss_finalize_groups (csrc/heads.hip): od_loss_finalize once per map of a validation group, one wave per map.

Rules:
  bit identity    out[g] equals, bit for bit, what od_loss_finalize returns on the rows of map g alone — groups of 1, 8, 63, 64, 65 and 130
                  rows (the last two take a second pass of the 64-lane loop), one row with dsq = 0, one with u equal to its target
  fp64            every value within 1e-6 relative of an fp64 evaluation of the formula on the same fp32 operands: fp32 rounding of the
                  per-row terms (a division, a square root: a few eps = 1.2e-7 each) and of a sum of at most 130 non-negative terms in a
                  three-level order (two or three per lane, then a 64-lane tree), which stays within ~10 eps
  fence           out lies in a NaN-fenced buffer; nothing outside it is written
  refusals        G = 0 and an empty map return OD_ERR_ARG (the row offsets are host integers: the launcher reads them)
  repeatability   two launches give identical bits
More maps than one launch carries (255) are covered too: the launcher splits them.
Emulator and MI355X (the `dev` fixture).
"""
import pytest
import torch

from osu_dreamer_amd import _lib, ops
from kernel_backend import Flat, bits, dev  # noqa: F401

C0, OSL_W, DEL_W = 0.5 ** 2 * 6, 1.0, 30.0
ROWS = (1, 8, 63, 64, 65, 130)
ERR_ARG = -1


def operands(rows, seed=0):
    """(sums (R, 3), dsq (R,), u (R,), offs) from seeded noise: sums[:, :2] and dsq are non-negative, as the kernels before this one
    leave them; row 2 has dsq = 0 and row 5 has u equal to its target sqrt(dsq + c0)."""
    gen = torch.Generator().manual_seed(seed)
    R = sum(rows)
    sums = torch.randn(R, 3, generator=gen)
    sums[:, :2] = sums[:, :2].square() * 4
    dsq = torch.randn(R, generator=gen).square() * 3
    dsq[2] = 0.0
    u = (dsq + C0).sqrt() * (1 + 0.3 * torch.randn(R, generator=gen))
    u[5] = (dsq[5] + C0).sqrt()
    offs = [0]
    for r in rows:
        offs.append(offs[-1] + r)
    return sums, dsq, u, offs


def fp64_formula(sums, dsq, u):
    sums, dsq, u = sums.double(), dsq.double(), u.double()
    den = dsq + C0                                             # (C0, OSL_W and DEL_W are exact in fp32)
    ut = den.sqrt()
    osl, dl, mape = (sums[:, 0] / den).mean(), sums[:, 1].mean(), ((u - ut) / ut).abs().mean()
    return torch.stack([OSL_W * osl + DEL_W * dl, osl, dl, mape])


def run_groups(sums, dsq, u, offs, dev):
    out = Flat((len(offs) - 1, 4), dev)
    ops.loss_finalize_groups(sums.to(dev), dsq.to(dev), u.to(dev), offs, out.v, C0, OSL_W, DEL_W)
    out.check("loss_finalize_groups", "out")
    return out.v.cpu()


def test_each_map_is_loss_finalize_on_its_rows_alone(dev):
    sums, dsq, u, offs = operands(ROWS)
    got = run_groups(sums, dsq, u, offs, dev)
    again = run_groups(sums, dsq, u, offs, dev)
    assert torch.equal(bits(got), bits(again)), "two launches differ"
    for g, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        alone, du = torch.empty(4, device=dev), torch.empty(b - a, device=dev)
        ops.loss_finalize(sums[a:b].contiguous().to(dev), dsq[a:b].contiguous().to(dev), u[a:b].contiguous().to(dev), alone, du, C0, OSL_W, DEL_W)
        assert torch.equal(bits(got[g]), bits(alone.cpu())), f"map {g} ({b - a} rows): {got[g].tolist()} against od_loss_finalize's {alone.tolist()}"
        want = fp64_formula(sums[a:b], dsq[a:b], u[a:b])
        rel = ((got[g].double() - want).abs() / want.abs()).max()
        print(f"map {g} ({b - a} rows): worst relative distance to fp64 {float(rel):.2e}")
        assert float(rel) <= 1e-6, (g, got[g].tolist(), want.tolist())
    assert float(got[:, 3].min()) > 0 and bool(torch.isfinite(got).all())


def test_more_maps_than_one_launch_carries(dev):
    rows = [1 + (i * 7) % 5 for i in range(600)]               # 600 maps: three launches (255 + 255 + 90)
    sums, dsq, u, offs = operands(rows, seed=1)
    got = run_groups(sums, dsq, u, offs, dev)
    for g in (0, 254, 255, 256, 509, 510, 599):
        a, b = offs[g], offs[g + 1]
        want = fp64_formula(sums[a:b], dsq[a:b], u[a:b])
        assert float(((got[g].double() - want).abs() / want.abs()).max()) <= 1e-6, g


def test_refusals(dev):
    sums, dsq, u, offs = operands((3, 4))
    sums, dsq, u = sums.to(dev), dsq.to(dev), u.to(dev)
    out = Flat((2, 4), dev)
    raw = _lib.lib().cdll.od_loss_finalize_groups

    def rc(offs, G):
        o = torch.tensor(offs, dtype=torch.int32)
        return raw(sums.data_ptr(), dsq.data_ptr(), u.data_ptr(), o.data_ptr(), out.v.data_ptr(), G, C0, OSL_W, DEL_W, 0)
    assert rc([0, 3, 7], 0) == ERR_ARG                          # G = 0
    assert rc([0, 3, 3], 2) == ERR_ARG                          # the second map is empty
    assert rc([0, 0, 7], 2) == ERR_ARG                          # the first one
    assert rc([0, 5, 3], 2) == ERR_ARG                          # rows that run backwards
    assert raw(sums.data_ptr(), dsq.data_ptr(), u.data_ptr(), None, out.v.data_ptr(), 2, C0, OSL_W, DEL_W, 0) == ERR_ARG
    assert bool(torch.isnan(out.buf).all()), "a refused call wrote"
    with pytest.raises(_lib.HipKernelError):
        ops.loss_finalize_groups(sums, dsq, u, [0, 3, 3], out.v, C0, OSL_W, DEL_W)
    with pytest.raises(AssertionError):
        ops.loss_finalize_groups(sums, dsq, u, [0, 3, 8], out.v, C0, OSL_W, DEL_W)      # rows u does not have
    assert rc([0, 3, 7], 2) == 0
    out.check("after the refusals", "out")
