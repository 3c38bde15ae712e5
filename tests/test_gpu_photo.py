"""lss_simbev_images_photo (colour jitter and sensor noise in the image kernel) against the numpy restatement of
tests/photo_cases.py applied to the Pillow restatement's pixels (oracle/simbev_ref.py). Bar: bit for bit -- the
resampled pixel is integer arithmetic, the photometric chain is fp32 operations rounded once each in a stated
order, the noise is integer Philox."""
import ctypes

import numpy as np
import pytest
import torch

import photo_cases as C

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from oracle import simbev_ref as S  # noqa: E402
from lss_carla_amd import _lib, simbev  # noqa: E402
from test_kernel_resources import _kernel_notes  # noqa: E402

DEV = torch.device("cuda:0")
SRC = C.sources(0)
NAMES = sorted(C.CASES)


@pytest.fixture(scope="module")
def reference():
    """name -> (u8 (3, fH, fW, 3) resampled pixels, inside (3, fH, fW) bool): computed once on the host."""
    out = {}
    white = np.full(C.SRC_HW + (3,), 255, dtype=np.uint8)
    for name, (fd, a) in C.CASES.items():
        args = (a["resize_dims"], a["crop"], a["flip"], a["rotate"])
        u8 = np.stack([S.img_transform(SRC[i], *args) for i in range(C.N_IMG)])
        lit = S.img_transform(white, *args)
        assert set(np.unique(lit)) <= {0, 255} and (lit == 255).any()
        inside = (lit == 255).all(axis=-1)
        assert np.array_equal(inside, (lit == 255).any(axis=-1))
        out[name] = (u8, np.stack([inside] * C.N_IMG))
    assert not out["crop_outside"][1].all() and not out["affine"][1].all() and out["copy_noresize"][1].all()
    return out


def _run(name, records):
    fd, a = C.CASES[name]
    photo = None if records is None else torch.from_numpy(np.stack(records))
    return simbev.augment_images(torch.from_numpy(SRC).to(DEV), [a] * C.N_IMG, fd, photo=photo)


def _expected(reference, name, records):
    u8, inside = reference[name]
    return np.stack([C.apply_photo(u8[i], inside[i], records[i], i) for i in range(C.N_IMG)])


COLOUR = [C.record(20.0, 1.3, 0.6, 12.0), C.record(-35.5, 0.7, 1.4, -18.0), C.record(0.0, 1.0, 0.0, 90.0)]
NOISY = [C.record(20.0, 1.3, 0.6, 12.0, 8.0, 0x12345678, 0x9ABCDEF0), C.record(0.0, 1.0, 1.0, 0.0, 2.5, 7, 0),
         C.record(-35.5, 0.7, 1.4, -18.0, 30.0, 0xFFFFFFFF, 0x7FC00001)]


@pytest.mark.parametrize("name", NAMES)
def test_neutral_records_are_the_plain_kernel(name):
    plain = _run(name, None)
    got = _run(name, [C.record()] * C.N_IMG)
    assert got.shape == plain.shape == (C.N_IMG, 3) + C.CASES[name][0] and torch.equal(got, plain)
    got = _run(name, [C.record(seed0=5, seed1=6)] * C.N_IMG)  # (a key without noise changes nothing)
    assert torch.equal(got, plain)


@pytest.mark.parametrize("name", NAMES)
def test_colour_only_bit_for_bit(reference, name):
    got = _run(name, COLOUR).cpu().numpy()
    want = _expected(reference, name, COLOUR)
    np.testing.assert_array_equal(got, want)
    u8, inside = reference[name]
    fill = np.stack([S.normalize_img(np.zeros_like(u8[0]))] * C.N_IMG)
    out = np.broadcast_to(~inside[:, None], got.shape)
    np.testing.assert_array_equal(got[out], fill[out])  # fill pixels stay the reference's black
    assert not np.array_equal(got, _run(name, None).cpu().numpy())


@pytest.mark.parametrize("name", ["affine", "crop_outside", "copy_flip_resize", "square_rot90"])
@pytest.mark.parametrize("delta, level", [(300.0, 255), (-300.0, 0)])
def test_brightness_past_the_range_clamps_every_inside_pixel(reference, name, delta, level):
    recs = [C.record(delta)] * C.N_IMG
    got = _run(name, recs).cpu().numpy()
    np.testing.assert_array_equal(got, _expected(reference, name, recs))
    u8, inside = reference[name]
    flat = np.where(inside[..., None], np.uint8(level), np.uint8(0)).astype(np.uint8)
    np.testing.assert_array_equal(got, np.stack([S.normalize_img(flat[i]) for i in range(C.N_IMG)]))


@pytest.mark.parametrize("name", NAMES)
def test_colour_and_noise_bit_for_bit(reference, name):
    got = _run(name, NOISY)
    np.testing.assert_array_equal(got.cpu().numpy(), _expected(reference, name, NOISY))
    assert torch.equal(got, _run(name, NOISY))  # the same seeds: the same output


def test_seed_and_sigma(reference):
    name = "affine_flip_upscale"
    base = _run(name, NOISY)
    other = [r.copy() for r in NOISY]
    other[1].view(np.uint32)[13] += 1
    got = _run(name, other)
    assert torch.equal(got[0], base[0]) and torch.equal(got[2], base[2]) and not torch.equal(got[1], base[1])
    np.testing.assert_array_equal(got.cpu().numpy(), _expected(reference, name, other))
    hi = [r.copy() for r in NOISY]
    hi[0].view(np.uint32)[14] ^= 0x80000000  # (the key's second word)
    assert not torch.equal(_run(name, hi)[0], base[0])
    quiet = [r.copy() for r in NOISY]
    for r, c in zip(quiet, COLOUR):
        r[:13] = c[:13]  # the colour records' matrices and noise = 0, the noisy ones' seeds
    assert torch.equal(_run(name, quiet), _run(name, COLOUR))
    # the same record for every image still draws a noise of its own per image (the index is in the counter)
    same = [NOISY[1]] * C.N_IMG
    np.testing.assert_array_equal(_run(name, same).cpu().numpy(), _expected(reference, name, same))


def test_c_abi_argument_checks():
    lib = _lib.load()
    fd, a = C.CASES["affine"]
    src = torch.from_numpy(SRC).to(DEV)
    buf = torch.zeros(64, device=DEV, dtype=torch.int32)
    out = torch.full((C.N_IMG, 3) + fd, 7.0, device=DEV)
    H, W = C.SRC_HW
    st = _lib.stream_handle(DEV)
    p = _lib.ptr
    assert lib.lss_simbev_images_photo(p(src), C.N_IMG, H, W, p(buf), None, p(buf), fd[0], fd[1], p(out), st) == -1
    assert lib.lss_simbev_images_photo(None, C.N_IMG, H, W, p(buf), p(buf), p(buf), fd[0], fd[1], p(out), st) == -1
    assert lib.lss_simbev_images_photo(p(src), C.N_IMG, H, W, p(buf), p(buf), p(buf), 0, fd[1], p(out), st) == -1
    assert lib.lss_simbev_images_photo(p(src), 65536, H, W, p(buf), p(buf), p(buf), fd[0], fd[1], p(out), st) == -2
    assert lib.lss_simbev_images(p(src), 65536, H, W, p(buf), p(buf), fd[0], fd[1], p(out), st) == -2
    torch.cuda.synchronize()
    assert (out == 7.0).all()  # nothing was launched
    with pytest.raises(RuntimeError, match="photo="):
        simbev.augment_images(src, [a] * C.N_IMG, fd, photo=torch.zeros(2, 16))
    with pytest.raises(RuntimeError, match="photo="):
        simbev.augment_images(src, [a] * C.N_IMG, fd, photo=torch.zeros(C.N_IMG, 16, dtype=torch.float64))
    assert ctypes.sizeof(_lib.ImgPhoto) == 64


def test_photo_instantiation_uses_no_scratch():
    kernels = {k: v for k, v in _kernel_notes(_lib.LIB_PATH).items() if "k_simbev_images" in k}
    assert len(kernels) == 2, sorted(kernels)  # the plain and the photo instantiation
    for name, v in kernels.items():
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 \
            and v.get("sgpr_spill_count", 0) == 0, (name, v)
