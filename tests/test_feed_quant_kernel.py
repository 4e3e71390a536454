"""od_feed_gather_quant (the resident beatmap feed's batch builder), on the emulator and on the MI355X (the `dev` fixture).

  q = store[base[n] + c * cstride[n] + l]                       unsigned integers of 1 or 2 bytes
  v = float32( float64(q) / qmax * scale[n][c] + offset[n][c] )   (no scale / offset: float32( float64(q) / qmax ))
  out[n][c0 + c][l] = l < lens[n] ? (bit c of flip[n] ? 1 - v : v) : 0

compared BIT FOR BIT with that formula in numpy float64 — the arithmetic of data.read_spec / data.read_beatmap followed by torch's .float()
and BeatmapDataset's `window[c].mul_(-1).add_(1)` — so there is no tolerance.  The output sits in a `Flat` buffer: NaN on entry (the zeros
must be selected and every element written) between NaN fences (nothing outside may be written).  The store tensor is allocated at exactly
the size a case needs, so the row that ends the store ends the allocation.
"""
import numpy as np
import pytest
import torch

from osu_dreamer_amd import _lib, ops
from kernel_backend import Flat, dev  # noqa: F401

QMAX = {1: 255.0, 2: 65535.0}
DT = {1: np.uint8, 2: np.uint16}
PAIRS = [(12.3456789, 487.654321), (0.0, 512.0), (-37.25, 401.7), (3.1, 0.37)]          # (offset, scale) = (xy_min, xy_rng)


def _ref_rows(q, es, scale=None, offset=None, flip=False):
    """The host loader's value of the codes q: float64 divide, multiply and add, each rounded; one rounding to fp32; the flip in fp32."""
    v = q.astype(np.float64) / QMAX[es]
    if scale is not None:
        v = v * scale + offset
    f = v.astype(np.float32)
    return np.float32(1) - f if flip else f


def _expected(codes, es, base, cstride, lens, C, Lpad, scale, offset, flip):
    out = np.zeros((len(lens), C, Lpad), dtype=np.float32)
    for n, (b, cs, ln) in enumerate(zip(base, cstride, lens)):
        for c in range(C):
            out[n, c, :ln] = _ref_rows(codes[b + c * cs: b + c * cs + ln], es, None if scale is None else scale[n, c],
                                       None if offset is None else offset[n, c], flip is not None and bool((flip[n] >> c) & 1))
    return out


def _dev(a, dtype, device):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, device=device)


def _launch(device, codes, es, base, cstride, lens, out, c0=0, channels=None, scale=None, offset=None, flip=None):
    """codes: numpy uint8 / uint16 (flat); the store is exactly their bytes."""
    st = torch.from_numpy(codes.view(np.uint8).copy()).to(device)
    ops.feed_gather_quant(st, es, _dev(base, torch.int64, device), _dev(cstride, torch.int64, device), _dev(lens, torch.int32, device), out,
                          c0=c0, channels=channels, scale=_dev(scale, torch.float64, device), offset=_dev(offset, torch.float64, device),
                          flip=_dev(flip, torch.int32, device))


def _run(device, codes, es, base, cstride, lens, C, Lpad, case, scale=None, offset=None, flip=None):
    """Asserts the gathered batch equals the numpy formula, bit for bit.  Returns the expected array."""
    assert codes.dtype == DT[es]
    out = Flat((len(lens), C, Lpad), device)         # NaN inside and 64 NaN elements either side
    _launch(device, codes, es, base, cstride, lens, out.v, scale=scale, offset=offset, flip=flip)
    out.check(case, "out")
    want = _expected(codes, es, base, cstride, lens, C, Lpad, scale, offset, flip)
    got = out.v.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), (case, np.argwhere(got.view(np.int32) != want.view(np.int32))[:4])
    return want


def _codes(n, es, seed):
    return np.random.default_rng(seed).integers(0, int(QMAX[es]) + 1, n, dtype=DT[es])


def _affine(N, C, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.3, 600.0, (N, C)), rng.uniform(-80.0, 80.0, (N, C))           # scale, offset


def test_one_element(dev):
    _run(dev, _codes(1, 1, 0), 1, [0], [1], [1], 1, 1, "u8 N=1 C=1 Lpad=1")
    _run(dev, _codes(1, 2, 1), 2, [0], [1], [1], 1, 1, "u16 N=1 C=1 Lpad=1", *_affine(1, 1, 2))


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_three_rows_seven_channels(dev, shift):
    """uint8, C = 7 (the hit signals), lens {1, 63, 130}, Lpad = 192; the three maps lie back to back behind `shift` bytes, so over the
    four shifts every row starts at every residue mod 4 (the dwords shifted by 0, 8, 16 and 24 bits)."""
    lens, C, Lpad = [1, 63, 130], 7, 192
    base, off = [], shift
    for ln in lens:
        base.append(off)
        off += C * ln
    _run(dev, _codes(off, 1, 1 + shift), 1, base, lens, lens, C, Lpad, f"3 rows shift {shift}")     # the last row's last channel ends the store


@pytest.mark.parametrize("es", [1, 2])
@pytest.mark.parametrize("Lpad", [5, 152])
def test_no_padding_and_odd_lpad(dev, Lpad, es):
    """len == Lpad (nothing to pad) beside a shorter row, at Lpad 5 (never a 16-byte store) and 152 = 4 * 38, every residue of the source.
    Windows of a longer map: cstride > len."""
    C, frames = 3, Lpad + 11
    for res in range(4):
        codes = _codes(res + C * frames, es, 7 * Lpad + res)
        _run(dev, codes, es, [res, res + 8], [frames, frames], [Lpad, max(1, Lpad - 3)], C, Lpad, f"es {es} Lpad {Lpad} res {res}",
             *(_affine(2, C, res) if es == 2 else ()))


def test_all_uint8_codes(dev):
    codes = np.arange(256, dtype=np.uint8)
    _run(dev, codes, 1, [0], [256], [256], 1, 256, "all 256 codes")
    _run(dev, codes, 1, [0], [256], [256], 1, 256, "all 256 codes, affine", *_affine(1, 1, 5))


@pytest.mark.parametrize("offset,scale", PAIRS)
def test_all_uint16_codes(dev, offset, scale):
    """Every uint16 code in one row of 65 536 frames (64 segments) under a realistic (xy_min, xy_rng), plain and flipped (1 - v after the
    rounding to fp32)."""
    codes = np.arange(65536, dtype=np.uint16)
    sc, of = np.array([[scale]]), np.array([[offset]])
    _run(dev, codes, 2, [0], [65536], [65536], 1, 65536, f"all uint16 codes at ({offset}, {scale})", sc, of)
    _run(dev, codes, 2, [0], [65536], [65536], 1, 65536, f"all uint16 codes flipped at ({offset}, {scale})", sc, of, np.array([1]))


def test_an_fp32_formula_is_not_the_reference():
    """The guard of the comparison above: evaluated in fp32, the same inputs do NOT give the reference's bits, so a kernel that computed
    in fp32 would fail test_all_uint16_codes.  This holds at three of the four pairs.  At (0, 512) the
    fp32 formula is exact by construction — a correctly rounded fp32 quotient of two integers below 2^24 is the fp64 quotient rounded to
    fp32 (q / 65535 is never within 2^-29 of an fp32 tie: its binary expansion repeats every 16 bits), the product with a power of two and
    the sum with zero do not round — so that pair checks the kernel's bits without telling the two formulas apart."""
    codes = np.arange(65536, dtype=np.uint16)
    differ = {}
    for offset, scale in PAIRS:
        want = _ref_rows(codes, 2, scale, offset)
        f32 = codes.astype(np.float32) / np.float32(65535) * np.float32(scale) + np.float32(offset)
        assert f32.dtype == np.float32
        differ[(offset, scale)] = int((f32.view(np.int32) != want.view(np.int32)).sum())
    print("outputs an fp32 formula changes, of 65536:", differ)
    assert all(n > 0 for pair, n in differ.items() if pair != (0.0, 512.0)), differ
    assert sum(differ.values()) > 0


@pytest.mark.parametrize("mask", [0, 1, 2, 3])
def test_flip_masks(dev, mask):
    """C = 2 (cursor x, y) under each of the four masks; the second row is padded (len 37 of 64) and its padding stays 0, flipped or not."""
    frames, Lpad = 90, 64
    codes = _codes(5 + 2 * frames, 2, 40 + mask)
    sc, of = _affine(2, 2, 41)
    want = _run(dev, codes, 2, [5, 11], [frames, frames], [64, 37], 2, Lpad, f"flip mask {mask}", sc, of, np.array([mask, mask]))
    assert not want[1, :, 37:].any()


def test_two_launches_fill_one_chart(dev):
    """hit (uint8, 7 channels, c0 = 0) and xy (uint16, 2 channels, c0 = 7, affine, flipped) into one (2, 9, 64) tensor: every element
    written once the two launches have run, none outside, and each launch leaves the other's channels alone."""
    frames, Lpad, lens = 80, 64, [64, 50]
    hit, xy = _codes(3 + 7 * frames, 1, 50), _codes(1 + 2 * frames, 2, 51)
    sc, of = _affine(2, 2, 52)
    flip = np.array([2, 1])
    out = Flat((2, 9, Lpad), dev)
    _launch(dev, hit, 1, [3, 10], [frames, frames], lens, out.v, c0=0, channels=7)
    assert bool(torch.isnan(out.v[:, 7:]).all()) and not bool(torch.isnan(out.v[:, :7]).any())
    _launch(dev, xy, 2, [1, 9], [frames, frames], lens, out.v, c0=7, channels=2, scale=sc, offset=of, flip=flip)
    out.check("chart", "out")
    want = np.concatenate([_expected(hit, 1, [3, 10], [frames, frames], lens, 7, Lpad, None, None, None),
                           _expected(xy, 2, [1, 9], [frames, frames], lens, 2, Lpad, sc, of, flip)], axis=1)
    assert np.array_equal(out.v.cpu().numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("es", [1, 2])
def test_row_ends_the_store(dev, es):
    """The row's last element is the store's last byte (the tensor is allocated at exactly that size), at every residue of the row's start
    and of its length: the dwords at the end of the store must not be read as dwords."""
    C, Lpad = 2, 64
    for res in range(4):
        for ln in (61, 62, 63, 64, 3, 1):
            frames = ln + res
            _run(dev, _codes(C * frames, es, 13 + res + ln), es, [res], [frames], [ln], C, Lpad, f"es {es} end of store res {res} len {ln}")
        for ln in (1, 2, 3, 5, 62):     # channels back to back (cstride = len): the store ends with the last channel's frame len - 1
            _run(dev, _codes(res + C * ln, es, 17 + ln), es, [res], [ln], [ln], C, Lpad, f"es {es} packed end of store res {res} len {ln}")


def test_more_than_one_segment_and_block(dev):
    """C = 72 (the spectrogram) over three rows of one mapset at different starts, Lpad beyond the 1024 frames a wave owns, padded from
    mid-segment."""
    C, frames, Lpad = 72, 1400, 1280
    _run(dev, _codes(C * frames + 3, 1, 23), 1, [0, 3, 121], [frames] * 3, [1280, 1100, 1025], C, Lpad, "C=72 Lpad 1280")


def test_descriptor_outside_the_store_is_not_loaded(dev):
    """A row whose descriptor reaches past the store (or has len outside 1..Lpad) is written as NaN and not loaded; its neighbours are
    gathered as usual."""
    C, Lpad = 2, 8
    codes = _codes(40, 2, 29)                                   # 80 bytes
    out = Flat((5, C, Lpad), dev)
    # row 1: channel 1 would end at 30 + 8 + 5 = 43 > 40; row 2: negative base; row 3: len > Lpad; row 4: a stride no store holds
    _launch(dev, codes, 2, [0, 30, -4, 0, 0], [8, 8, 8, 8, 2 ** 62], [8, 5, 4, 9, 4], out.v)
    got = out.v.cpu()
    assert np.array_equal(got[0].numpy(), _ref_rows(codes[:16], 2).reshape(2, 8))
    assert np.array_equal(got[1, 0, :5].numpy(), _ref_rows(codes[30:35], 2)) and bool((got[1, 0, 5:] == 0).all())     # channel 0 lies inside
    assert bool(torch.isnan(got[1, 1]).all()) and bool(torch.isnan(got[2]).all()) and bool(torch.isnan(got[3]).all())
    assert bool(torch.isnan(got[4]).all())
    assert bool(torch.isnan(out.buf[:64]).all() & torch.isnan(out.buf[64 + out.n:]).all())


def test_bad_arguments(dev):
    st = torch.zeros(16, dtype=torch.uint8, device=dev)
    i64 = torch.zeros(1, dtype=torch.int64, device=dev)
    i32 = torch.ones(1, dtype=torch.int32, device=dev)
    f64 = torch.ones(1, 1, dtype=torch.float64, device=dev)
    out = torch.empty(1, 1, 4, device=dev)
    L = _lib.lib()
    p = lambda t: None if t is None else t.data_ptr()

    def call(store=st, nbytes=16, es=1, base=i64, scale=None, offset=None, C=1, c0=0, Ctot=1, Lpad=4):
        L.od_feed_gather_quant(p(store), nbytes, es, p(base), i64.data_ptr(), i32.data_ptr(), p(scale), p(offset), None, out.data_ptr(),
                               1, C, c0, Ctot, Lpad, 0)

    call()                                                        # the arguments the refusals below vary are valid
    for bad in (dict(store=None), dict(base=None), dict(Lpad=0), dict(es=4), dict(es=0), dict(scale=f64), dict(offset=f64), dict(c0=1),
                dict(c0=-1, Ctot=4), dict(nbytes=0)):
        with pytest.raises(_lib.HipKernelError, match="code -1"):  # OD_ERR_ARG
            call(**bad)
    with pytest.raises(AssertionError):
        ops.feed_gather_quant(st.float(), 1, i64, i64, i32, out)
    with pytest.raises(AssertionError):
        ops.feed_gather_quant(st, 1, i64, i64, i32, out, scale=f64)


@pytest.mark.gpu
def test_row_beyond_2_pow_31():
    """Rows read from beyond byte 2^31 of an uninitialised 2.2 GB store (a real store is tens of GB): uint8 and uint16, only those rows'
    sources are filled; the second uint16 row ends the store."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _lib._lib = None
    _lib.lib()
    device = torch.device("cuda:0")
    free, _ = torch.cuda.mem_get_info(device)
    if free < 4 * 2 ** 30:
        pytest.skip("less than 4 GB of device memory free")
    C, frames, ln, Lpad = 2, 1000, 130, 192
    first = 2 ** 31 + 12345                                     # bytes; odd: the uint8 rows start off a dword
    first16 = (first + C * frames + 1) // 2                     # elements of 2 bytes behind the uint8 map
    store = torch.empty(2 * first16 + 2 * C * frames, dtype=torch.uint8, device=device)        # never initialised
    u8, u16 = _codes(C * frames, 1, 31), _codes(C * frames, 2, 32)
    store[first:first + C * frames].copy_(torch.from_numpy(u8))
    store[2 * first16:].copy_(torch.from_numpy(u16.view(np.uint8)))
    i64 = lambda a: torch.tensor(a, dtype=torch.int64, device=device)
    lens = torch.tensor([ln, ln], dtype=torch.int32, device=device)
    out = Flat((2, 2 * C, Lpad), device)
    ops.feed_gather_quant(store, 1, i64([first + 7, first + frames - ln]), i64([frames, frames]), lens, out.v, c0=0, channels=C)
    sc, of = _affine(2, C, 33)
    ops.feed_gather_quant(store, 2, i64([first16 + 7, first16 + frames - ln]), i64([frames, frames]), lens, out.v, c0=C, channels=C,
                          scale=torch.from_numpy(sc).to(device), offset=torch.from_numpy(of).to(device))
    out.check("beyond 2^31", "out")
    want = np.concatenate([_expected(u8, 1, [7, frames - ln], [frames, frames], [ln, ln], C, Lpad, None, None, None),
                           _expected(u16, 2, [7, frames - ln], [frames, frames], [ln, ln], C, Lpad, sc, of, None)], axis=1)
    assert np.array_equal(out.v.cpu().numpy().view(np.int32), want.view(np.int32))
    del store
    torch.cuda.empty_cache()
