"""od_feed_gather (the resident feed's batch builder), on the emulator and on the MI355X (the `dev` fixture).

out[n][c][l] = l < len[n] ? store[base[n] + c * cstride[n] + l] : 0, compared BIT FOR BIT with a numpy slice-and-pad: the kernel only
copies, so there is no tolerance.  The output buffer is NaN on entry (the zeros must be selected and every element written) and sits
between NaN fences (nothing outside it may be written).  The store is NaN everywhere a case must not read — between and behind the rows'
channels when `cstride` is wider than the rows — so a load at or past len[n] shows up in the output only if it is also stored; the over-read
itself is what the row that ends exactly at the store's last element is for (the store tensor is allocated at exactly that size).
"""
import numpy as np
import pytest
import torch

from osu_dreamer_amd import _lib, ops
from kernel_backend import Flat, dev  # noqa: F401


def _expected(store, base, cstride, lens, C, Lpad):
    out = np.zeros((len(lens), C, Lpad), dtype=np.float32)
    for n, (b, cs, ln) in enumerate(zip(base, cstride, lens)):
        for c in range(C):
            out[n, c, :ln] = store[b + c * cs: b + c * cs + ln]
    return out


def _run(device, store, base, cstride, lens, C, Lpad, case):
    """store: numpy fp32 (flat).  Returns nothing: asserts the gathered batch equals the slice-and-pad, bit for bit."""
    N = len(lens)
    st = torch.from_numpy(store).to(device)
    out = Flat((N, C, Lpad), device)                 # NaN inside and 64 NaN elements either side
    ops.feed_gather(st, torch.tensor(base, dtype=torch.int64, device=device), torch.tensor(cstride, dtype=torch.int64, device=device),
                    torch.tensor(lens, dtype=torch.int32, device=device), out.v)
    out.check(case, "out")
    want = _expected(store, base, cstride, lens, C, Lpad)
    got = out.v.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), (case, np.argwhere(got.view(np.int32) != want.view(np.int32))[:4])


def _store(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def test_one_element(dev):
    _run(dev, _store(1, 0), [0], [1], [1], 1, 1, "N=1 C=1 Lpad=1")


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_three_rows_six_channels(dev, shift):
    """N = 3, C = 6, lens {1, 63, 130}, Lpad = 192; the three maps lie back to back behind `shift` elements, so over the four shifts every
    row starts at every residue mod 4 (the 16-byte path where the source is aligned, the dword path elsewhere)."""
    lens, C, Lpad = [1, 63, 130], 6, 192
    base, off = [], shift
    for ln in lens:
        base.append(off)
        off += C * ln
    store = _store(off, 1 + shift)                  # the last row's last channel ends the store
    _run(dev, store, base, lens, lens, C, Lpad, f"3 rows shift {shift}")


@pytest.mark.parametrize("Lpad", [5, 64, 152])
@pytest.mark.parametrize("res", [0, 1, 2, 3])
def test_no_padding_and_odd_lpad(dev, Lpad, res):
    """len == Lpad (nothing to pad) beside a shorter row, at Lpad 5 and 152 (152 = 4 * 38 takes the 16-byte path only when the source is
    aligned; 5 never does) and base = res mod 4.  Windows of a longer map: cstride > len."""
    C, frames = 3, Lpad + 11
    store = _store(res + C * frames, 7 * Lpad + res)
    base = [res, res + 8]                           # both = res mod 4
    lens = [Lpad, max(1, Lpad - 3)]
    _run(dev, store, base, [frames, frames], lens, C, Lpad, f"Lpad {Lpad} res {res}")


def test_two_windows_of_one_mapset(dev):
    """Two rows from the SAME mapset's h (one stored copy) at different starts, one of them overlapping the other."""
    C, frames, Lpad = 4, 300, 128
    store = _store(C * frames, 11)
    _run(dev, store, [16, 101], [frames, frames], [128, 77], C, Lpad, "shared h")


@pytest.mark.parametrize("res", [0, 1, 2, 3])
def test_row_ends_the_store(dev, res):
    """The last channel of the row ends exactly at the last element of the store tensor (allocated at exactly that size), with the valid
    length at every residue mod 4 relative to an aligned and an unaligned start: the quad that straddles len must be peeled, not loaded."""
    C, Lpad = 2, 64
    for ln in (61, 62, 63, 64, 3):
        frames = ln + res
        store = _store(C * frames, 13 + res + ln)
        _run(dev, store, [res], [frames], [ln], C, Lpad, f"end of store res {res} len {ln}")
    # and an aligned source whose valid frames stop mid-quad at the very end of the store (the 16-byte path's peel)
    for ln in (1, 2, 3, 5, 62):
        # channel 0 at element 8 (aligned), channel 1 directly behind it: cstride = ln; the store ends with channel 1's frame ln - 1
        _run(dev, _store(8 + C * ln, 17 + ln), [8], [ln], [ln], C, Lpad, f"aligned end of store len {ln}")


def test_wide_channels(dev):
    """C = 128 (the width of h) with cstride larger than Lpad, more than one block, rows of one map at an aligned and an unaligned start."""
    C, frames, Lpad = 128, 411, 192
    store = _store(C * frames + 5, 19)
    _run(dev, store, [0, 5, 219], [frames, frames, frames], [192, 130, 192], C, Lpad, "C=128")


def test_more_than_one_segment(dev):
    """Lpad beyond the 1024 frames one wave owns: the row's second and third segment, aligned and unaligned, padded from mid-segment."""
    C, frames, Lpad = 2, 2500, 2304
    store = _store(C * frames + 3, 23)
    _run(dev, store, [0, 3, 4], [frames] * 3, [2304, 2100, 1025], C, Lpad, "Lpad 2304")


def test_bad_arguments(dev):
    st = torch.zeros(16, device=dev)
    i64 = torch.zeros(1, dtype=torch.int64, device=dev)
    i32 = torch.ones(1, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.HipKernelError, match="code -1"):             # OD_ERR_ARG: a null store
        ops.feed_gather(torch.empty(0, device=dev), i64, i64, i32, torch.empty(1, 1, 4, device=dev))
    L = _lib.lib()
    out = torch.empty(1, 1, 4, device=dev)
    with pytest.raises(_lib.HipKernelError, match="code -1"):             # Lpad < 1
        L.od_feed_gather(st.data_ptr(), 16, i64.data_ptr(), i64.data_ptr(), i32.data_ptr(), out.data_ptr(), 1, 1, 0, 0)
    with pytest.raises(_lib.HipKernelError, match="code -1"):             # null descriptors
        L.od_feed_gather(st.data_ptr(), 16, None, i64.data_ptr(), i32.data_ptr(), out.data_ptr(), 1, 1, 4, 0)


def test_descriptor_outside_the_store_is_not_loaded(dev):
    """A row whose descriptor reaches past the store (or has len outside 1..Lpad) is written as NaN and not loaded; its neighbours are
    gathered as usual."""
    C, Lpad = 2, 8
    store = _store(40, 29)
    st = torch.from_numpy(store).to(dev)
    out = Flat((5, C, Lpad), dev)
    base = torch.tensor([0, 30, -4, 0, 0], dtype=torch.int64, device=dev)   # row 1: channel 1 would end at 30 + 8 + 5 = 43 > 40
    cstride = torch.tensor([8, 8, 8, 8, 2 ** 62], dtype=torch.int64, device=dev)       # row 4: a stride no store holds
    lens = torch.tensor([8, 5, 4, 9, 4], dtype=torch.int32, device=dev)    # row 3: len > Lpad
    ops.feed_gather(st, base, cstride, lens, out.v)
    got = out.v.cpu()
    assert np.array_equal(got[0].numpy(), store[:16].reshape(2, 8))
    assert np.array_equal(got[1, 0, :5].numpy(), store[30:35]) and bool((got[1, 0, 5:] == 0).all())     # channel 0 lies inside
    assert bool(torch.isnan(got[1, 1]).all()) and bool(torch.isnan(got[2]).all()) and bool(torch.isnan(got[3]).all())
    assert bool(torch.isnan(got[4]).all())
    assert bool(torch.isnan(out.buf[:64]).all() & torch.isnan(out.buf[64 + out.n:]).all())


@pytest.mark.parametrize("C, stride", [(5, 2 ** 62), (9, 2 ** 61)])
def test_a_stride_whose_product_wraps_is_not_gathered(dev, C, stride):
    """(C - 1) * stride = 2^64 wraps to 0: the last channel's offset would pass a test made after the product and gather channel 0's
    frames.  The stride is checked against the store first, so the whole row is NaN; its ordinary neighbour is gathered bit for bit.
    Nothing outside the 64-element store is loaded either way."""
    Lpad = 8
    store = _store(64, 37)
    st = torch.from_numpy(store).to(dev)
    out = Flat((2, C, Lpad), dev)
    ops.feed_gather(st, torch.tensor([1, 3], dtype=torch.int64, device=dev), torch.tensor([7, stride], dtype=torch.int64, device=dev),
                    torch.tensor([6, 4], dtype=torch.int32, device=dev), out.v)
    got = out.v.cpu().numpy()
    want = _expected(store, [1], [7], [6], C, Lpad)
    assert np.array_equal(got[:1].view(np.int32), want.view(np.int32))
    assert np.isnan(got[1]).all(), np.argwhere(~np.isnan(got[1]))[:4]
    assert bool(torch.isnan(out.buf[:64]).all() & torch.isnan(out.buf[64 + out.n:]).all())


@pytest.mark.gpu
def test_row_beyond_2_pow_31():
    """One row gathered from beyond element 2^31 of an uninitialised store: only that row's source is filled."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _lib._lib = None
    _lib.lib()
    device = torch.device("cuda:0")
    free, _ = torch.cuda.mem_get_info(device)
    if free < 12 * 2 ** 30:
        pytest.skip("less than 12 GB of device memory free")
    C, frames, ln, Lpad = 6, 1000, 130, 192
    first = 2 ** 31 + 12345                                  # channel 0 of the map: beyond what a 32-bit offset reaches
    store = torch.empty(first + C * frames, device=device)   # 8.6 GB, never initialised
    src = torch.randn(C, frames, generator=torch.Generator().manual_seed(31))
    store[first:].copy_(src.reshape(-1))
    out = Flat((2, C, Lpad), device)
    base = torch.tensor([first + 7, first + frames - ln], dtype=torch.int64, device=device)    # the second row's last channel ends the store
    ops.feed_gather(store, base, torch.tensor([frames, frames], dtype=torch.int64, device=device),
                    torch.tensor([ln, ln], dtype=torch.int32, device=device), out.v)
    out.check("beyond 2^31", "out")
    want = torch.zeros(2, C, Lpad)
    want[0, :, :ln], want[1, :, :ln] = src[:, 7:7 + ln], src[:, frames - ln:]
    assert torch.equal(out.v.cpu().view(torch.int32), want.view(torch.int32))
    del store
    torch.cuda.empty_cache()
