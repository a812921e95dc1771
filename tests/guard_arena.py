"""One allocation, many buffers, a known bit pattern everywhere else.

tests/test_gpu_guards.py carves every buffer a kernel WRITES out of such an arena: a store outside an output changes the pattern.
tests/test_gpu_input_guards.py carves every buffer a kernel READS out of one as well and changes the pattern between runs: a
result that depends on memory outside its operands changes with it.  The 256 KB guard in front of and behind every buffer keeps a
read or a write that is a few tiles off inside the one allocation.

Three fill words, each one int32 pattern that means the same thing as fp32, as a bf16 pair and as an fp16 pair:

    NEG0       0x80000000   fp32 -0.0 (an fp32 atomic add of +0.0 flips the sign: the invisible kind of stray write)
    NAN_WORD   0x7FC07FC0   NaN in all three: anything multiplied, added or exponentiated shows
    HUGE_WORD  0x7B007B00   6.67e35 / 6.65e35 / 57344: finite and huge, shows where a max / min or a compare swallows a NaN
"""
import torch

NEG0 = -2147483648          # 0x80000000 as int32
NAN_WORD = 0x7FC07FC0
HUGE_WORD = 0x7B007B00
FILLS = (('neg0', NEG0), ('nan', NAN_WORD), ('huge', HUGE_WORD))


def _i32(word):
    word &= 0xFFFFFFFF
    return word - (1 << 32) if word >= (1 << 31) else word


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _esize(dtype):
    return torch.empty((), dtype=dtype).element_size()


class GuardArena:
    """One int32 allocation of fill words (fp32 -0.0 unless given); build() returns tensors of it separated by guard zones (also one
    in front of the first and one behind the last); check() verifies every word outside the taken ranges.

    plan(name, shape, dtype): a dense buffer.  plan(name, (rows, cols), dtype, ld, col): a 2-D view at column offset `col` of rows
    that are `ld` elements apart -- the column slice of a wider buffer.  Every element of those rows outside the view is a gap
    word, checked like the guards.  (col, cols and ld must be whole 32-bit words.)
    refill(word) rewrites every guard and gap word and leaves the taken ranges alone."""

    def __init__(self, guard_bytes=1 << 18, fill=NEG0, device='cuda'):
        self.guard = guard_bytes // 4
        self.fill = _i32(fill)
        self.device = device
        self.req = []

    def plan(self, name, shape, dtype, ld=None, col=0):
        shape = tuple(shape)
        if ld is not None:
            es = _esize(dtype)
            if len(shape) != 2 or col < 0 or col + shape[1] > ld:
                raise ValueError(f'{name}: a strided slot is a 2-D view inside rows of ld elements')
            if (col * es) % 4 or (shape[1] * es) % 4 or (ld * es) % 4:
                raise ValueError(f'{name}: col, width and ld must be whole 32-bit words')
            if ld == shape[1]:
                ld = None
        elif col:
            raise ValueError(f'{name}: a column offset needs ld')
        self.req.append((name, shape, dtype, ld, col))

    @staticmethod
    def _used_words(shape, dtype, ld):
        n = _numel(shape) if ld is None else shape[0] * ld
        return (n * _esize(dtype) + 3) // 4

    def build(self):
        off = self.guard
        self.slots = {}
        for name, shape, dtype, ld, col in self.req:
            words = self._used_words(shape, dtype, ld)
            words = (words + 63) // 64 * 64          # 256-byte aligned starts
            self.slots[name] = (off, words, shape, dtype, ld, col)
            off += words + self.guard
        self.buf = torch.full((off,), self.fill, dtype=torch.int32, device=self.device)
        out = {}
        for name, (o, w, shape, dtype, ld, col) in self.slots.items():
            flat = self.buf[o:o + w].view(dtype)
            if ld is None:
                out[name] = flat[:_numel(shape)].view(shape)
            else:
                out[name] = flat[:shape[0] * ld].view(shape[0], ld)[:, col:col + shape[1]]
        return out

    def _keep(self):
        """True at every word that belongs to no buffer: guards, alignment tails and the gaps of strided slots"""
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        for name, (o, w, shape, dtype, ld, col) in self.slots.items():
            if ld is None:
                keep[o:o + self._used_words(shape, dtype, None)] = False
            else:
                es = _esize(dtype)
                wpr = ld * es // 4
                keep[o:o + shape[0] * wpr].view(shape[0], wpr)[:, col * es // 4:(col + shape[1]) * es // 4] = False
        return keep

    def refill(self, word):
        self.fill = _i32(word)
        self.buf[self._keep()] = self.fill

    def check(self, what):
        bad = (self.buf != self.fill) & self._keep()
        if bool(bad.any()):
            idx = int(torch.nonzero(bad)[0])
            near = [nm for nm, (o, w, *_r) in self.slots.items() if o - self.guard <= idx < o + w + self.guard]
            gap = [nm for nm, (o, w, shape, dtype, ld, col) in self.slots.items()
                   if ld is not None and o <= idx < o + self._used_words(shape, dtype, ld)]
            where = f'gap word {idx} inside the rows of strided slot {gap[0]!r}' if gap else f'guard word {idx}'
            raise AssertionError(f'{what}: {where} changed ({int(bad.sum())} words in all); nearest buffer(s): {near}')
