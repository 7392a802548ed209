"""Guard-band arenas of the region-product kernel tests (helper of tests/test_gpu_kernel_matrix.py and
tests/test_gpu_gf_geometry.py; numpy only apart from `to_dev`, imports nothing of the project).

An arena is a [stripes][slots][pitch] uint8 image: every B-byte block sits between two 64-byte bands of 0xC3 at a
16-byte-aligned pitch.  Input blocks hold seeded random bytes; the blocks of an output arena, named by the op or not,
hold 0x3C.  A test uploads the image, makes its call, and compares the whole arena with the expected image, so a store
past a block's end and a store into a block the op does not name both show.
"""
import numpy as np

GUARD, BAND, FILL = 64, 0xC3, 0x3C


def pitch(B):
    return (GUARD + B + GUARD + 15) & ~15  # every block 16-byte aligned in an aligned arena


def blank(stripes, slots, B, fill=FILL):
    """[stripes][slots][pitch(B)] image: bands of BAND, every block filled with `fill`."""
    img = np.full((stripes, slots, pitch(B)), BAND, np.uint8)
    img[:, :, GUARD:GUARD + B] = fill
    return img


def blocks(img, B):
    """The [stripes][slots][B] view of an image's (or a device tensor's) blocks."""
    return img[:, :, GUARD:GUARD + B]


def to_dev(torch, img, shift=0):
    """The image on the device, its base `shift` bytes past a 16-byte boundary."""
    flat = torch.empty(img.size + 16, dtype=torch.uint8, device="cuda")
    view = flat[shift:shift + img.size]
    view.copy_(torch.from_numpy(img.reshape(-1)))
    return view.view(img.shape)


def where(idx, shape, B, written):
    """What lies at flat index idx of an arena if the op may not write there, else None.  written(s, slot): the op
    names that block as an output."""
    s, slot, off = (int(v) for v in np.unravel_index(idx, shape))
    if off < GUARD or off >= GUARD + B:
        return f"guard band of stripe {s} slot {slot} at byte {off - GUARD} of the block"
    if not written(s, slot):
        return f"untouched block: stripe {s} slot {slot} byte {off - GUARD}"
    return None


def assert_same(got, want, B, written, label, describe=None):
    """got == want over the whole arena; the failure names a byte written outside the op's output blocks first, else
    the first wrong byte (describe(s, slot, o) may add to it)."""
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    outside = [w for w in (where(i, got.shape, B, written) for i in bad[:4096]) if w]
    assert not outside, (label, f"{len(bad)} bytes differ; written outside the named blocks", outside[:4])
    s, slot, off = (int(v) for v in np.unravel_index(bad[0], got.shape))
    msg = describe(s, slot, off - GUARD) if describe else ""
    raise AssertionError(f"{label}: {len(bad)} bytes differ; first at stripe {s} slot {slot} byte {off - GUARD}: "
                         f"got {got[s, slot, off]:#04x}, want {want[s, slot, off]:#04x} {msg}")
