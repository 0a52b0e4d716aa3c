"""Guarded device buffers for the poison tests (tests/test_gpu_poison.py): one allocation laid out guard | payload | guard.

The guards hold a fixed NaN bit pattern and are compared bit for bit after a call (check_guards); the payload is filled with
zeros, with that NaN pattern, or with seeded finite junk (+-U(0.5, 1e3), random signs) before it.  Every guard is 64 KiB, so a
ragged last tile that reads past its operand stays inside the allocation: an over-read shows up in the results, an over-write
in the guards, and neither can become a fault.  The payload starts 256 bytes into an allocation-aligned block (align=256), or
16 bytes past such a boundary (align=16: aligned to 16 bytes and to nothing wider)."""
import torch

NAN_BITS = 0x7FC0DEAD               # a quiet NaN no kernel produces by arithmetic
GUARD = 64 << 10                    # bytes of guard on each side
FILLS = ("zero", "nan", "junk")
DEV = "cuda:0"


def junk_like(n, seed, device=DEV):
    """n seeded finite floats +-U(0.5, 1e3) with random signs"""
    g = torch.Generator(device=device).manual_seed(seed)
    mag = torch.rand(n, generator=g, device=device) * (1e3 - 0.5) + 0.5
    sign = torch.randint(0, 2, (n,), generator=g, device=device, dtype=torch.int32) * 2 - 1
    return mag * sign


def fill_words(words, fill, seed=0):
    """fill an int32 view with a fill pattern (the float payload's bits)"""
    if fill == "zero":
        words.zero_()
    elif fill == "nan":
        words.fill_(NAN_BITS)
    elif fill == "junk":
        words.copy_(junk_like(words.numel(), seed, words.device).view(torch.int32))
    else:
        raise ValueError(fill)


class Guarded:
    """n_words 4-byte words of payload (float32 by default) between two NaN-filled guards"""

    def __init__(self, n_words, fill="zero", align=256, seed=0, dtype=torch.float32, device=DEV):
        assert align in (16, 256)
        self.n = int(n_words)
        self.off = (GUARD + (0 if align == 256 else 16)) // 4          # payload offset in words
        total = self.off + self.n + (256 + GUARD) // 4
        self.raw = torch.empty(total, dtype=torch.int32, device=device)
        self.raw.fill_(NAN_BITS)
        self.words = self.raw[self.off:self.off + self.n]
        self.dtype = dtype
        self.fill(fill, seed)

    def fill(self, fill, seed=0):
        fill_words(self.words, fill, seed)
        return self

    @property
    def t(self):
        """the payload as a flat tensor of the buffer's dtype"""
        return self.words.view(self.dtype)

    @property
    def ptr(self):
        return self.raw.data_ptr() + 4 * self.off

    def set(self, values):
        """copy values (any shape, 4-byte dtype) into the start of the payload"""
        v = values.reshape(-1).to(self.raw.device).contiguous().view(torch.int32)
        self.words[:v.numel()].copy_(v)
        return self

    def view(self, *shape):
        n = 1
        for s in shape:
            n *= s
        return self.t[:n].view(*shape)

    def snapshot(self):
        """bits of the whole allocation (guards and payload)"""
        return self.raw.clone()

    def check_guards(self, what):
        lo, hi = self.raw[:self.off], self.raw[self.off + self.n:]
        bad_lo = int((lo != NAN_BITS).sum())
        bad_hi = int((hi != NAN_BITS).sum())
        assert bad_lo == 0 and bad_hi == 0, f"{what}: {bad_lo} guard words before and {bad_hi} after the payload changed"

    def check_unchanged(self, snap, what):
        diff = int((self.raw != snap).sum())
        assert diff == 0, f"{what}: {diff} words of a const buffer (or its guards) changed"


def poison_gaps(words, covered, total, fill="nan", seed=0):
    """fill the elements of a flat parameter buffer (int32 view, `total` words) that no tensor covers - the padding between
    tensors and the round-up to 4: covered = [(offset, numel), ...]"""
    mask = torch.ones(total, dtype=torch.bool, device=words.device)
    for off, n in covered:
        mask[off:off + n] = False
    tmp = torch.empty(total, dtype=torch.int32, device=words.device)
    fill_words(tmp, fill, seed)
    words[:total][mask] = tmp[mask]
    return mask


def bits_equal(a, b):
    """bit-for-bit equality of two float tensors (NaN payloads included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
