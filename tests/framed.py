"""Frames: an operand as a strided view in the middle of one allocation that is otherwise sentinel memory.

A kernel that indexes with the padded width where it should use the leading dimension, a tile that overruns the
padded shape, a store into the [width, ld) gap of a row, a workspace used past its stated size, or an input that is
written after all, changes words the test owns and compares -- it is detected, not faulted on.

Layout of the one buffer (in elements of `dtype`, nexp experts of rows x cols):

    [ front guard: >= row_guard * ld, ending `lead` elements past a 256-byte boundary ]
    [ expert 0: rows x ld, the last ld - cols of every row are the gap ][ batch_gap ]
    [ expert 1: ...                                                    ][ batch_gap ] ...
    [ back guard: row_guard * ld ]

so the view's base pointer is 16-byte but not 256-byte aligned (what `base + e * stride` and `work + n * n` look like
inside a real caller) and its row stride is cols + gap.  1-D operands, int32 info words and workspaces are frames of
shape (n,); a workspace frame is exactly the stated size.  Every word starts as one fixed quiet-NaN bit pattern and all
comparisons are on the integer view of the memory, never on floats.

Works on CPU tensors too (tests/test_framed_cpu.py drives it with NumPy stand-ins through `.numpy()`)."""
import numpy as np
import torch

SENTINEL64 = 0x7FF85EA75EA75EA7       # quiet NaN, fp64
SENTINEL32 = 0x7FC5EA75               # quiet NaN, fp32 (and the pattern of an untouched int32 word)
ROW_GUARD = 256                       # the tallest tile any kernel stores (csrc/gemm.hip: 128 x 128 and 256 x 128 C tiles;
                                      # kbuild.hip / kmfma.hip: 128; leaf / chainstep: 128-row panels)
_WORD = {8: torch.int64, 4: torch.int32}
_SENT = {8: SENTINEL64, 4: SENTINEL32}


class FrameError(AssertionError):
    """What a check found: `kind` (guard / changed / unwritten), `count` of offending words, `where` = (expert, row, column) of the
    first one relative to the view (row < 0: front guard; row >= rows: between experts or back guard; column >= cols: the gap),
    and `region` in {front, gap, between, back, view}."""

    def __init__(self, name, kind, count, where, region):
        self.name, self.kind, self.count, self.where, self.region = name, kind, int(count), tuple(int(v) for v in where), region
        super().__init__("%s: %s -- %d word(s), first at (expert %d, row %d, column %d) [%s]" % ((name, kind, self.count) + self.where + (region,)))


class Frame:
    def __init__(self, shape, dtype, device, gap=0, row_guard=ROW_GUARD, lead=None, batch_gap=0, name="operand"):
        shape = tuple(int(s) for s in shape)
        assert 1 <= len(shape) <= 3
        self.name, self.shape, self.dtype = name, shape, dtype
        self.item = torch.empty(0, dtype=dtype).element_size()
        assert self.item in _WORD
        self.nexp = shape[0] if len(shape) == 3 else 1
        self.rows = shape[-2] if len(shape) >= 2 else 1
        self.cols = shape[-1]
        self.ld = self.cols + int(gap)
        self.estride = self.rows * self.ld + int(batch_gap)
        self.lead = 16 // self.item if lead is None else int(lead)
        per256 = 256 // self.item
        guard = int(row_guard) * max(self.ld, 1)
        self.start = ((guard + per256 - 1) // per256) * per256 + self.lead
        self.span = (self.nexp - 1) * self.estride + (self.rows - 1) * self.ld + self.cols      # first to last element of the view
        self.total = self.start + self.nexp * self.estride + guard
        self.buf = torch.empty(self.total, dtype=dtype, device=device)
        self.words = self.buf.view(_WORD[self.item])
        self.words.fill_(_SENT[self.item])
        sizes, strides = {1: ((self.cols,), (1,)), 2: ((self.rows, self.cols), (self.ld, 1)),
                          3: ((self.nexp, self.rows, self.cols), (self.estride, self.ld, 1))}[len(shape)]
        self.view = torch.as_strided(self.buf, sizes, strides, self.start)
        self.wview = torch.as_strided(self.words, sizes, strides, self.start)
        self._snap = None

    # -- addresses ----------------------------------------------------------------------------
    @property
    def ptr(self):
        return self.view.data_ptr()

    def inside(self):
        """Boolean mask over the whole buffer: True for the words of the view."""
        m = torch.zeros(self.total, dtype=torch.bool, device=self.buf.device)
        torch.as_strided(m, self.wview.shape, self.wview.stride(), self.start).fill_(True)
        return m

    def locate(self, off):
        """(expert, row, column), region of a flat offset into the buffer."""
        rel = int(off) - self.start
        if rel < 0:
            return (0, rel // self.ld, rel % self.ld), "front"      # floor division: row -1 is the row just before the view
        e = min(rel // self.estride, self.nexp - 1)
        within = rel - e * self.estride
        row, col = within // self.ld, within % self.ld
        if row < self.rows:
            return (e, row, col), ("gap" if col >= self.cols else "view")
        return (e, row, col), ("between" if e < self.nexp - 1 else "back")

    def _raise(self, kind, bad):
        idx = torch.nonzero(bad.reshape(-1), as_tuple=False)
        where, region = self.locate(int(idx[0]))
        raise FrameError(self.name, kind, idx.shape[0], where, region)

    # -- contents -----------------------------------------------------------------------------
    def fill(self, data):
        """Copy `data` (NumPy or tensor of the view's shape) into the view; the gaps and guards keep the sentinel."""
        t = torch.as_tensor(np.array(data)) if not torch.is_tensor(data) else data
        self.view.copy_(t.reshape(self.view.shape).to(self.buf.device, self.dtype))
        return self

    def poison(self, mask):
        """NaN (an ordinary one, not the sentinel) wherever the boolean `mask` (view-shaped) is set: parts the header says are not read."""
        m = torch.as_tensor(np.array(mask)).reshape(self.view.shape).to(self.buf.device)
        self.view.masked_fill_(m, float("nan")) if self.dtype.is_floating_point else self.view.masked_fill_(m, -0x5EA75EA8)
        return self

    def packed(self):
        """The same logical contents as a fresh contiguous tensor (the operand of the reference call on packed memory)."""
        return self.view.clone().contiguous()

    def bits(self):
        return self.wview.cpu().numpy().copy()

    # -- checks -------------------------------------------------------------------------------
    def check_guards(self):
        bad = (self.words != _SENT[self.item]) & ~self.inside()
        if bool(bad.any()):
            self._raise("guard overwritten", bad)

    def snapshot(self):
        self._snap = self.words.clone()
        return self

    def check_unchanged(self, except_mask=None):
        """Bitwise equal to the snapshot, the gaps and guards included.  `except_mask` (view-shaped): entries the call may write."""
        assert self._snap is not None, "snapshot() first"
        bad = self.words != self._snap
        if except_mask is not None:
            ok = torch.zeros(self.total, dtype=torch.bool, device=self.buf.device)
            m = torch.as_tensor(np.array(except_mask)).reshape(self.view.shape).to(self.buf.device)
            torch.as_strided(ok, self.wview.shape, self.wview.stride(), self.start).copy_(m)
            bad &= ~ok
        if bool(bad.any()):
            self._raise("changed", bad)

    def check_written(self, mask=None):
        """No sentinel left where the call writes (`mask`, view-shaped boolean; None: the whole view)."""
        bad = self.wview == _SENT[self.item]
        if mask is not None:
            bad = bad & torch.as_tensor(np.array(mask)).reshape(self.view.shape).to(self.buf.device)
        if bool(bad.any()):
            full = torch.zeros(self.total, dtype=torch.bool, device=self.buf.device)
            torch.as_strided(full, self.wview.shape, self.wview.stride(), self.start).copy_(bad)
            self._raise("left unwritten", full)


def frame(shape, dtype, device, gap=0, row_guard=ROW_GUARD, lead=None, batch_gap=0, name="operand"):
    return Frame(shape, dtype, device, gap=gap, row_guard=row_guard, lead=lead, batch_gap=batch_gap, name=name)


def min_gap(dtype):
    """The smallest gap that keeps rows 16-byte aligned: 2 elements fp64, 4 fp32."""
    return 16 // torch.empty(0, dtype=dtype).element_size()
