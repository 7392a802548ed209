"""CRC-32C (Castagnoli) by its definition, with no table or constant from the product: the reflected CRC with
polynomial 0x1EDC6F41 (reflected constant 0x82F63B78), initial value 0xFFFFFFFF and final XOR 0xFFFFFFFF.

`bitwise` is the definition, one bit at a time.  `many` is a numpy form for tests that need the sums of many blocks:
it walks the byte positions once, all blocks at a time, with a 256-entry table that is generated from `bitwise`'s own
step.
"""
import numpy as np

POLY = 0x82F63B78

KNOWN = (
    (b"123456789", 0xE3069283),
    (bytes(32), 0x8A9136AA),
    (b"\xff" * 32, 0x62A8AB43),
    (bytes(range(32)), 0x46DD794E),
    (bytes(range(31, -1, -1)), 0x113FDB5C),
    (b"\x00", 0x527D5351),
    (b"", 0),
)


def _step(reg):
    """One bit: the register times x."""
    return (reg >> 1) ^ (POLY if reg & 1 else 0)


def bitwise(data):
    reg = 0xFFFFFFFF
    for byte in bytes(data):
        reg ^= byte
        for _ in range(8):
            reg = _step(reg)
    return reg ^ 0xFFFFFFFF


def _table():
    t = np.zeros(256, dtype=np.uint32)
    for v in range(256):
        reg = v
        for _ in range(8):
            reg = _step(reg)
        t[v] = reg
    return t


TABLE = _table()


def many(blocks, lengths=None):
    """crc32c of every row of `blocks` ([..., B] uint8): a uint32 array of shape blocks.shape[:-1].  lengths (same
    shape, integers in [0, B]): row r is summed over its first lengths[r] bytes only."""
    blocks = np.asarray(blocks, dtype=np.uint8)
    reg = np.full(blocks.shape[:-1], 0xFFFFFFFF, dtype=np.uint32)
    out = reg.copy()
    for x in range(blocks.shape[-1]):
        reg = TABLE[(reg ^ blocks[..., x]) & np.uint32(0xFF)] ^ (reg >> np.uint32(8))
        if lengths is not None:
            out = np.where(np.asarray(lengths) == x + 1, reg, out)
    return (reg if lengths is None else out) ^ np.uint32(0xFFFFFFFF)
