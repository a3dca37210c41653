"""Guarded arena for tests of the C ABI: one uint8 allocation filled with byte 0xFF from which a case carves every tensor a
kernel sees (inputs, outputs, workspaces, device tables, scalars) as contiguous views at 256-byte aligned starts.

0xFF bytes are NaN as fp32, bf16 and e4m3fn, -1 as int32 and 255 as uint8, so
  * the guards on both sides of every tensor are NaN: a read past an input that reaches arithmetic poisons the result;
  * outputs and workspaces start as NaN: "fully overwritten" and "no slot read before it is written" are `not isnan`;
  * check() finds every byte written outside a tensor and names the tensor, the side and the offset.

Guard size is a condition, not a measurement: on each side of a tensor at least GUARD_ROWS rows of its innermost row (the
tallest tile any kernel of the library owns is 128 rows) and at least GUARD_MIN bytes.  A tensor's last byte is followed
directly by guard bytes.  Works on CPU tensors too (tests/test_abi_arena.py)."""
import torch

POISON = 0xFF
ALIGN = 256
GUARD_ROWS = 128
GUARD_MIN = 64 * 1024
FLAT_ROW = 8192         # elements taken as the "row" of a 1-D tensor longer than this (flat kernels own at most 256 x 4 x 8 a block)


class ArenaError(AssertionError):
    pass


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


class Arena:
    def __init__(self, device, mib=64):
        self.buf = torch.full((int(mib) << 20,), POISON, dtype=torch.uint8, device=device)
        self.device = self.buf.device
        self.top = 0            # first byte not yet promised to a tensor or to the guard behind one
        self.regions = []       # (name, start, end, guard) in address order
        self.dtypes = []        # regions[i]'s element type: what a poison byte there means (NaN as a float, an index as an int)

    # ---- carving
    def guard_bytes(self, shape, dtype):
        row = int(shape[-1]) if len(shape) >= 2 else min(int(shape[0]) if len(shape) else 1, FLAT_ROW)
        return max(GUARD_ROWS * max(row, 1) * _itemsize(dtype), GUARD_MIN)

    def empty(self, name, shape, dtype):
        """a poisoned (all 0xFF) contiguous tensor with guards of guard_bytes() on both sides"""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        n = 1
        for s in shape:
            n *= s
        nbytes = n * _itemsize(dtype)
        g = self.guard_bytes(shape, dtype)
        base = self.buf.data_ptr()
        start = self.top + g if not self.regions else max(self.top, self.regions[-1][2] + g)
        start += (-(base + start)) % ALIGN
        end = start + nbytes
        if end + g > self.buf.numel():
            raise ArenaError(f"arena of {self.buf.numel()} bytes is too small for {name} {shape} ({end + g} bytes needed)")
        self.regions.append((name, start, end, g))
        self.dtypes.append(dtype)
        self.top = end + g
        t = self.buf[start:end].view(dtype).view(shape)
        assert t.is_contiguous() and t.data_ptr() % ALIGN == 0
        return t

    def put(self, name, src):
        """a copy of `src` (any device) inside the arena"""
        t = self.empty(name, src.shape, src.dtype)
        t.copy_(src)
        return t

    def zeros(self, name, shape, dtype):
        return self.fill(self.empty(name, shape, dtype), 0)

    @staticmethod
    def bytes_of(t):
        return t.reshape(-1).view(torch.uint8)

    @classmethod
    def fill(cls, t, byte=POISON):
        """every byte of the arena tensor `t` set to `byte`"""
        cls.bytes_of(t).fill_(byte)
        return t

    @classmethod
    def untouched(cls, t):
        return bool((cls.bytes_of(t) == POISON).all())

    # ---- checking
    def check(self):
        """raises ArenaError if a byte outside the carved tensors is no longer 0xFF (synchronise first on a GPU)"""
        bad = self.buf != POISON
        for _, s, e, _ in self.regions:
            bad[s:e] = False
        if not bool(bad.any()):
            return
        idx = bad.nonzero().flatten()
        first, count = int(idx[0]), int(idx.numel())
        where = []
        for name, s, e, g in self.regions:
            if s - g <= first < s:
                where.append(f"{s - first} bytes before the start of '{name}'")
            if e <= first < e + g:
                where.append(f"{first - e} bytes after the end of '{name}'")
        raise ArenaError(f"{count} guard bytes overwritten, first at arena offset {first} (value {int(self.buf[first])}): "
                         + ("; ".join(where) if where else "outside every guard"))
