"""Operands whose blocks lie far apart in one large device allocation: block offsets at and above 2^31 and 2^32 elements.

Every product record of the multiply packs its operand offsets as 40 bits (Entry in dbcsr_amd/csrc/mm_types.h: a_lo, b_lo and bits 32-39 of both in
bits 16-23 / 24-31 of w).  A packed matrix of a few MB never sets one of the upper bits.  Here a host matrix is given far block offsets (place), copied
block by block into an arena of 2^36 + 2^26 bytes that is never filled as a whole (Far.on_device), and read back block by block (blocks_to_host).

arena(nbytes)        one torch.empty(nbytes, uint8) per test module, viewed as float32 / float64 / complex128: high bytes 0 ... 4 / 0 ... 2 / 0 ... 1.
                     ARENA_LARGE = 2^36 + 2^26 bytes when the device has that much free plus MARGIN, else ARENA_SMALL = 2^35 + 2^26, else None (the
                     cases skip).  MARGIN is twice the largest torch.cuda.max_memory_allocated() over the arena that a module of the far tests reached
                     on an MI355X (profiles/far_offsets.txt).
place(M, dtype, plan, who)
                     pure numpy: int64 element offsets for M's blocks.  Zone 0 is the arena's start, zone z >= 1 surrounds the z-th of the boundaries
                     2^29, 2^31, 2^32, 2^32 + 2^31, 2^33, 2^34, ... elements that the view reaches.  A zone has three slots of SLOT elements: one below
                     the boundary, one around it, one above it.  The slot around it belongs to A (who 0) in odd zones and to B (who 1) in even ones, and
                     exactly one block of that matrix begins below the boundary and ends above it; the other two matrices take the slots below and above.
                     who exchanges the roles: a multiply with A placed as who 1 and B as who 0 gives the other matrix the straddling blocks.
                     plan "lines": a whole block row (A, C_in) or block column (B) goes to zone (line + who) mod Z, so every product of a C block has the
                     same (a_hi, b_hi); plan "blocks": block b goes to zone (5 b + who) mod Z, so the high bytes vary inside every product list.
                     plan "ascending": the blocks go to the zones in index order, a Z-th of them each, so blk_p ascends with the block index (the
                     lab's group kernels take no other B: mm_group64.hip, group_check_ascending).
Far(view)            one multiply's (or one check's) matrices on the device: on_device copies the blocks and writes CANARY into GUARD elements on either
                     side of every run of blocks; seal() fills with NaN the places a wrong decode of an offset >= 2^32 would read instead (the offset
                     modulo 2^32 under every other high byte), where no block or guard lives; guards_kept() compares every guard bit for bit.
blocks_to_host(dM)   the blocks of a device matrix, by slices of its data area, as a packed host matrix (never to_host() on a far matrix: that copies
                     the arena)."""
import numpy as np

ARENA_LARGE = 2 ** 36 + 2 ** 26
ARENA_SMALL = 2 ** 35 + 2 ** 26
# twice the 160 585 216 bytes that torch.cuda.max_memory_allocated() reached over the arena in the whole module of the far tests on an MI355X -- a bound on its
# largest case (profiles/far_offsets.txt)
MARGIN = 2 * 160585216
SLOT = 2 ** 20       # elements per slot of a zone
GUARD = 1024         # canary elements on either side of a run of blocks
CANARY = -77.25      # (CANARY of tests/test_gpu_multivec.py)
TWO32 = 2 ** 32


def boundaries(nelem):
    """the element offsets 2^29, 2^31, 2^32, 2^32 + 2^31, 2^33, 2^33 + 2^31, 2^34, ... with room for a zone's upper slots below nelem (2^33 + 2^31: so that
    both operands have whole lines with high byte 2 in a float32 view)"""
    cand = [2 ** 29, 2 ** 31, 2 ** 32, 2 ** 32 + 2 ** 31, 2 ** 33, 2 ** 33 + 2 ** 31] + [2 ** k for k in range(34, 40)]
    return [b for b in cand if b + 2 * SLOT <= nelem]


def view_elements(dtype, nbytes):
    return int(nbytes) // np.dtype(dtype).itemsize


def block_sizes(M):
    return M.row_sizes[M.rows()].astype(np.int64) * M.col_sizes[M.col_i].astype(np.int64)


def place(M, dtype, plan, who, nbytes=ARENA_LARGE, lines=None):
    """far blk_p of the host matrix M (see the module's text).  lines: "row" / "col", what plan "lines" keeps together (default: columns for who 1)"""
    bnd = boundaries(view_elements(dtype, nbytes))
    Z = len(bnd) + 1
    assert Z % 5 != 0 and who in (0, 1, 2) and plan in ("lines", "blocks", "ascending")
    size = block_sizes(M)
    if plan == "ascending":
        zone = np.arange(M.nblks, dtype=np.int64) * Z // max(1, M.nblks)
    elif plan == "lines":
        lines = lines or ("col" if who == 1 else "row")
        line = M.rows().astype(np.int64) if lines == "row" else M.col_i.astype(np.int64)
        zone = (line + who) % Z
    else:
        zone = (5 * np.arange(M.nblks, dtype=np.int64) + who) % Z
    out = np.full(M.nblks, -1, np.int64)
    for z in range(Z):
        idx = np.flatnonzero(zone == z)
        if idx.size == 0:
            continue
        owner = 0 if z % 2 == 1 else 1
        j = None
        if z > 0 and who == owner:
            # the run that straddles the boundary: its lines in order, the first half of them below the boundary and the rest above it, so that a line
            # keeps one high byte; the straddling block is the last one of the last line below (it begins below: its offset has that line's high byte)
            key = line[idx] if plan == "lines" else idx
            idx = idx[np.argsort(key, kind="stable")]
            key = key[np.argsort(key, kind="stable")]
            uniq = np.unique(key)
            members = np.flatnonzero(key == uniq[(len(uniq) - 1) // 2])
            cand = members[size[idx[members]] >= 2]
            if cand.size:
                j = int(members[-1])
                idx[[int(cand[-1]), j]] = idx[[j, int(cand[-1])]]
            else:
                cand = np.flatnonzero(size[idx] >= 2)
                j = int(cand[np.argmin(np.abs(cand - int(members[-1])))]) if cand.size else None
        lens = size[idx]
        before = np.concatenate([[0], np.cumsum(lens)[:-1]])
        total = int(lens.sum())
        assert total + 2 * GUARD + 2 <= SLOT, "a zone's share of the matrix must fit a slot"
        if z == 0:
            start = who * SLOT + GUARD
        else:
            b = bnd[z - 1]
            odd = 1 if z % 4 in (1, 2) else 0   # the slots below and above start at odd elements in half of the zones
            if who == owner:
                start = b - int(lens[j]) // 2 - int(before[j]) if j is not None else b - total
            else:
                below = (z % 2 == 0) != (who == 2)   # A or B beside the other's straddling run: above in odd zones, below in even ones; C_in opposite
                start = (b - 2 * SLOT if below else b + SLOT) + GUARD + odd
        out[idx] = start + before
    return out


def straddlers(M, blk_p, boundary):
    """the blocks that begin below the boundary and end above it"""
    size = block_sizes(M)
    return np.flatnonzero((blk_p < boundary) & (blk_p + size > boundary))


def runs_of(blk_p, size):
    """[(start, end, blocks in ascending offset)] of the maximal runs of adjacent blocks"""
    order = np.argsort(blk_p, kind="stable")
    out = []
    for b in order:
        s, e = int(blk_p[b]), int(blk_p[b] + size[b])
        if e == s:
            continue
        if out and out[-1][1] == s:
            out[-1][1] = e
            out[-1][2].append(int(b))
        else:
            out.append([s, e, [int(b)]])
    return [(s, e, bs) for s, e, bs in out]


def overlaps(intervals):
    """True when two of the half-open intervals share an element"""
    iv = sorted((int(s), int(e)) for s, e in intervals if e > s)
    return any(iv[i][1] > iv[i + 1][0] for i in range(len(iv) - 1))


def subtract(window, taken):
    """the pieces of the half-open window that none of the (sorted, disjoint) intervals covers"""
    s, e = window
    out = []
    for ts, te in taken:
        if te <= s or ts >= e:
            continue
        if ts > s:
            out.append((s, ts))
        s = max(s, te)
        if s >= e:
            break
    if s < e:
        out.append((s, e))
    return out


def alias_windows(runs, nelem):
    """where a decode that loses or swaps the high byte would read the parts of the runs at or above 2^32: the offset modulo 2^32 under every other
    high byte the view has"""
    out = []
    for s, e in runs:
        s = max(s, TWO32)
        while s < e:
            cut = min(e, (s // TWO32 + 1) * TWO32)
            for h in range(0, (nelem - 1) // TWO32 + 1):
                if h != s // TWO32:
                    a = s % TWO32 + h * TWO32
                    out.append((a, min(a + (cut - s), nelem)))
            s = cut
    return [(a, b) for a, b in out if b > a]


# ---- the device side ------------------------------------------------------------------------------------------------------------------------------------
class Arena:
    def __init__(self, nbytes):
        import torch
        self.nbytes = int(nbytes)
        self.bytes = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")

    def view(self, dtype):
        import torch
        t = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.complex128): torch.complex128}[np.dtype(dtype)]
        return self.bytes.view(t)

    def release(self):
        import torch
        del self.bytes
        torch.cuda.empty_cache()


def arena(nbytes=None):
    """the largest of ARENA_LARGE / ARENA_SMALL that the device has free besides MARGIN (or exactly nbytes), None when neither fits"""
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    for n in ([nbytes] if nbytes else [ARENA_LARGE, ARENA_SMALL]):
        if free >= n + MARGIN:
            return Arena(n)
    return None


class Far:
    """the far matrices of one multiply or check in one view of the arena"""

    def __init__(self, view):
        self.view = view
        self.nelem = int(view.numel())
        self.blocks = []    # (start, end) of every run of blocks
        self.guards = []    # (start, end) of every canary window

    def on_device(self, M, blk_p_far, symmetry="N"):
        import torch
        from dbcsr_amd.matrix import DbcsrMatrix
        blk_p_far = np.ascontiguousarray(blk_p_far, np.int64)
        size = block_sizes(M)
        assert blk_p_far.shape == (M.nblks,) and M.data.dtype == np.dtype(str(self.view.dtype).replace("torch.", ""))
        runs = runs_of(blk_p_far, size)
        guards = []
        for s, e, _ in runs:
            assert 0 <= s and e <= self.nelem, "a block outside the arena"
            guards += [(max(0, s - GUARD), s), (e, min(self.nelem, e + GUARD))]
        assert not overlaps(self.blocks + self.guards + [(s, e) for s, e, _ in runs] + guards), "blocks or guards of two matrices overlap"
        for s, e, blks in runs:
            host = np.concatenate([M.data[M.blk_p[b]:M.blk_p[b] + size[b]] for b in blks])
            self.view[s:e].copy_(torch.from_numpy(host))
        for s, e in guards:
            self.view[s:e].fill_(CANARY)
        self.blocks += [(s, e) for s, e, _ in runs]
        self.guards += guards
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
        dM = DbcsrMatrix(t(M.row_sizes, torch.int32), t(M.col_sizes, torch.int32), t(M.row_p, torch.int32), t(M.col_i, torch.int32),
                         t(blk_p_far, torch.int64), self.view, symmetry=symmetry, nze=int(size.sum()))
        return dM

    def seal(self):
        """NaN where a wrong high byte would read, except where a block or a guard of this set lives"""
        taken = sorted(self.blocks + self.guards)
        n = 0
        for w in alias_windows(self.blocks, self.nelem):
            for s, e in subtract(w, taken):
                self.view[s:e].fill_(float("nan"))
                n += 1
        return n

    def guards_kept(self):
        """every canary window still holds CANARY, bit for bit"""
        import torch
        if not self.guards:
            return True
        got = torch.cat([self.view[s:e] for s, e in self.guards]).cpu().numpy()
        return got.tobytes() == np.full(got.shape, CANARY, got.dtype).tobytes()

    def max_high_byte(self):
        return max((e - 1) // TWO32 for _, e in self.blocks) if self.blocks else 0


def blocks_to_host(dM):
    """packed host matrix (oracle.Bcsr) of the blocks the device matrix's index names: copied run by run, never the whole data area"""
    import torch
    from oracle import oracle as O
    g = lambda t: t.detach().cpu().numpy()
    rs, cs, row_p, col_i, blk_p = g(dM.row_blk_size), g(dM.col_blk_size), g(dM.row_p), g(dM.col_i), g(dM.blk_p).astype(np.int64)
    rows = np.repeat(np.arange(len(rs)), np.diff(row_p))
    size = rs[rows].astype(np.int64) * cs[col_i].astype(np.int64)
    packed_p = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64) if len(size) else np.zeros(0, np.int64)
    runs = runs_of(blk_p, size)
    npdt = np.dtype(str(dM.data.dtype).replace("torch.", ""))
    if not runs:
        return O.Bcsr(rs, cs, row_p, col_i, packed_p, np.zeros(0, npdt))
    got = torch.cat([dM.data[s:e] for s, e, _ in runs]).cpu().numpy()
    data = np.empty(int(size.sum()), npdt)
    at = 0
    for s, e, blks in runs:
        for b in blks:
            data[packed_p[b]:packed_p[b] + size[b]] = got[at:at + size[b]]
            at += int(size[b])
    return O.Bcsr(rs, cs, row_p, col_i, packed_p, data)
