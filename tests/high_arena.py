"""Arenas whose offsets pass 2^32: layouts, sentinel arenas and a host model of the classic
32-bit truncations, for test_gpu_high_offsets.py (the GPU runs) and test_high_arena_layout.py
(the conditions that keep those runs from passing by accident, checked without a GPU).

Every batch call takes 64-bit element offsets (sym_off, out_off, code_off).  A kernel that
keeps one of them, or the byte address it scales it to, in 32 bits is right on every arena
below 4 GiB and wrong above.  The layouts here put a handful of small chunks around the byte
offset 2^32 of an arena that is otherwise nothing but sentinels, so that

  - a truncated read finds sentinels (bytes the oracle does not produce from them), and
  - a truncated write lands where untouched() counts it.

One launch cannot hold every placement at once: sym_off and out_off are n + 1 entries, so the
chunks of a launch are contiguous, and either one chunk holds the boundary in its interior
(mode "straddle") or one chunk ends on it and the next begins on it (mode "exact").  The case
table gives every family both: one direction runs its symbol arena in one mode, the other
direction in the other (PLACEMENTS / CASES below).  Decoder input is addressed per stream
(code_off): code_layout() shuffles the streams, lays one across the boundary and the rest
either far below it or above it.

Pure numpy and Python; torch is touched only inside the functions under "device side"."""
import numpy as np

BOUNDARY = 1 << 32
SLICE_BYTES = 256 << 20   # untouched() compares at most this much per step
TAIL_BYTES = 4096         # sentinels past the last element a layout uses (at least)
MEM_CAP = 24 << 30        # peak device memory of one GPU test

# The chunk lengths every family runs (tests' parity lengths) and a few random ones.
BASE_LENS = [0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 300]


def chunk_lens(seed=1, n=40):
    """About n chunk lengths: BASE_LENS three times over in a shuffled order, then random ones."""
    rng = np.random.default_rng(seed)
    lens = BASE_LENS * 3
    lens = lens + [int(x) for x in rng.integers(2, 200, n - len(lens))]
    lens = np.array(lens, np.int64)
    rng.shuffle(lens)
    return lens


# ------------------------------------------------------------------------------- placements
# name -> (element bytes, the byte offset the layouts are laid around, what passes 2^32 there).
# "byte": the byte offset; "index": the element index as well.
PLACEMENTS = {
    "u8": (1, 1 << 32, ("byte", "index")),         # 8-bit symbols, idx, slots, code
    "u16": (2, 1 << 32, ("byte",)),                # 16-bit symbols: element 2^31
    "u16_index": (2, 1 << 33, ("byte", "index")),  # 16-bit symbols: element 2^32 (8 GiB)
    "row_of": (4, 1 << 32, ("byte",)),             # a row index per symbol: element 2^30
    "triples": (12, 1 << 32, ("byte",)),           # (c, cum, total): element 2^32 // 12
}


def _pivot(lens, need):
    """The chunk that sits on the boundary: the first of at least `need` symbols at or past
    a third of the list, so that the chunks after it (at least a third) lie wholly above."""
    n = len(lens)
    for p in range(n // 3, n - (n + 2) // 3):
        if lens[p] >= need:
            return p
    raise ValueError(f"no chunk of {need} symbols in the middle third of {list(lens)}")


def layout(lens, elem_bytes, boundary_bytes=BOUNDARY, phase=None, mode="straddle"):
    """Element offsets off (int64, len(lens) + 1) of contiguous chunks around the byte offset
    boundary_bytes of an arena of elem_bytes-byte elements.

    mode "straddle": one chunk begins below the boundary and ends above it.
    mode "exact": one non-empty chunk ends exactly on the boundary and the next non-empty one
    begins exactly on it (elem_bytes must divide the boundary).
    In both, off[0] * elem_bytes lies below the boundary and at least a third of the chunks lie
    wholly above it.  phase (straddle only): off[0] * elem_bytes % 64, so a test can keep the
    head lengths another test's layout has; the straddling chunk is cut where that holds."""
    lens = np.asarray(lens, np.int64)
    eb = int(elem_bytes)
    rel = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    if mode == "exact":
        if boundary_bytes % eb:
            raise ValueError("no element begins on the boundary")
        if phase is not None:
            raise ValueError("an exact layout leaves no freedom for a phase")
        n = len(lens)
        p = next((p for p in range(max(n // 3, 1), n - (n + 2) // 3)
                  if lens[p] > 0 and lens[p - 1] > 0), None)
        if p is None:
            raise ValueError("no two adjacent non-empty chunks in the middle third")
        base = boundary_bytes // eb - rel[p]
    elif mode == "straddle":
        step = 64 // np.gcd(64, eb)  # element steps after which the phase repeats
        p = _pivot(lens, 2 if phase is None else step + 1)
        first_above = -(-boundary_bytes // eb)  # the first element that begins at or past it
        # cut: the chunk's elements [0, cut) begin below the boundary, 1 <= cut < its length
        cut = int(lens[p]) // 2 if phase is None else None
        if phase is not None:
            for j in range(1, int(lens[p])):
                if ((first_above - j - rel[p]) * eb) % 64 == phase % 64:
                    cut = j
                    break
            if cut is None:
                raise ValueError(f"phase {phase} cannot be had with {eb}-byte elements")
        assert 1 <= cut < lens[p]
        base = first_above - cut - rel[p]
    else:
        raise ValueError(mode)
    if base < 0:
        raise ValueError("the chunks before the boundary do not fit below it")
    return rel + base


def slot_layout(caps, boundary_bytes=BOUNDARY, mode="straddle"):
    """(out_off, caps) for encoder slots of caps bytes each: out_off (int64, len(caps) + 1)
    contiguous around the boundary as layout() places chunks, with an odd out_off[0].  Slot 0
    is grown by one byte where that is what makes the start odd; the caps returned are the ones
    laid out."""
    caps = np.array(caps, np.int64)
    off = layout(caps, 1, boundary_bytes, mode=mode)
    if off[0] % 2 == 0:
        caps[0] += 1
        off = layout(caps, 1, boundary_bytes, mode=mode)
    assert off[0] % 2 == 1
    return off, caps


def code_layout(code_lens, seed=0, boundary_bytes=BOUNDARY, low_base=1 << 20,
                high_span=1 << 18):
    """code_off (int64, one per stream, not monotone) for decoder input of code_lens bytes each:
    the first eighth of the streams at low offsets (from low_base), one stream across the
    boundary, and the rest above it in shuffled order at every alignment mod 16, each in a slot
    of its own with at least 64 sentinels before the next.  Everything above the boundary lies
    within high_span bytes of it and low_base lies past high_span, so a high offset taken mod
    2^32 falls into the sentinels below the low streams."""
    code_lens = np.asarray(code_lens, np.int64)
    n = len(code_lens)
    order = np.random.default_rng(seed).permutation(n)
    n_low = max(n // 8, 1)
    off = np.zeros(n, np.int64)

    def slot(k):
        return 64 * ((int(code_lens[k]) + 16 + 63) // 64 + 1)

    pos = low_base
    for j, k in enumerate(order[:n_low]):
        off[k] = pos + j % 16
        pos += slot(k)
    rest = [int(k) for k in order[n_low:]]
    across = next((k for k in rest if code_lens[k] >= 2), None)
    if across is None:
        raise ValueError("need a stream of at least 2 bytes to lay across the boundary")
    off[across] = boundary_bytes - int(code_lens[across]) // 2
    pos = boundary_bytes + slot(across)
    j = 0
    for k in rest:
        if k == across:
            continue
        off[k] = pos + j % 16
        j += 1
        pos += slot(k)
    if pos + 64 > boundary_bytes + high_span or low_base < high_span:
        raise ValueError("the streams above the boundary pass high_span")
    return off


FILLER_BYTES = (1 << 32) + 4103  # the code length the containers' chunk 0 claims


def filler_layout(caps, filler_bytes=FILLER_BYTES):
    """slot_off (int64, len(caps) + 1) for the container cases: slot 0 begins 16-byte aligned
    (one wave copies it, 16 bytes a lane) and is filler_bytes long, whatever caps[0] says, so
    every other slot lies past the boundary; the others are contiguous behind it, the first of
    them at an odd offset."""
    caps = np.array(caps, np.int64)
    assert caps[0] <= filler_bytes
    caps[0] = filler_bytes
    off = 16 + np.concatenate([[0], np.cumsum(caps)])
    if off[1] % 2 == 0:
        off[1:] += 1
    return off


def arena_elems(last_elem, elem_bytes):
    """Elements of an arena whose layouts use elements below last_elem: TAIL_BYTES of sentinels
    past them (the decoders load whole aligned 16-byte segments around a stream's last byte, and
    the existing helpers keep 16 to 64 elements there), rounded up to 64 elements."""
    pad = -(-TAIL_BYTES // int(elem_bytes)) + 64
    return int(-(-(int(last_elem) + pad) // 64) * 64)


def truncations(off, elem_bytes, bits=32):
    """The byte address each chunk start off[k] would get under the three classic mistakes, as
    a dict of int64 arrays (the true address is off * elem_bytes):
      "byte_mod": the byte offset taken mod 2^32;
      "byte_sext": the byte offset's low 32 bits sign-extended;
      "index_mod": the element index taken mod 2^32 before scaling."""
    off = np.asarray(off, np.int64)
    eb, m = int(elem_bytes), 1 << bits
    true = off * eb
    mod = true % m
    sext = np.where(mod >= m // 2, mod - m, mod)
    return {"byte_mod": mod, "byte_sext": sext, "index_mod": (off % m) * eb}


def merged(ranges):
    """Sorted, non-empty, non-overlapping [a, b) ranges with adjacent ones joined."""
    out = []
    for a, b in sorted((int(a), int(b)) for a, b in ranges if b > a):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [(a, b) for a, b in out]


# ------------------------------------------------------------------------------- device side
def _sentinel(dtype, sentinel):
    """The sentinel as a value of the tensor's dtype (int16 holds 16-bit symbols bit for bit)."""
    import torch
    if dtype == torch.int16:
        return int(np.uint16(sentinel & 0xFFFF).view(np.int16))
    if dtype == torch.int32:
        return int(np.uint32(sentinel & 0xFFFFFFFF).view(np.int32))
    return int(sentinel)


def arena(n_elems, dtype, sentinel):
    """A device tensor of n_elems elements (place_elems() or arena_elems(): the layout and its
    tail of sentinels) filled with the sentinel."""
    import torch
    return torch.full((int(n_elems),), _sentinel(dtype, sentinel), dtype=dtype, device="cuda")


def put(t, start, values):
    """values (numpy) into t[start:], bit for bit."""
    import torch
    v = np.ascontiguousarray(values)
    if not v.size:
        return
    if v.dtype == np.uint16:
        v = v.view(np.int16)
    elif v.dtype == np.uint32:
        v = v.view(np.int32)
    t[int(start):int(start) + v.size] = torch.from_numpy(v).to(t.device)


def window(t, a, b):
    """t[a:b] on the host, as unsigned where the tensor holds symbols or rows bit for bit."""
    h = t[int(a):int(b)].cpu().numpy()
    return h.view({np.dtype(np.int16): np.uint16, np.dtype(np.int32): np.uint32}.get(
        h.dtype, h.dtype))


def untouched(t, keep_ranges, sentinel):
    """The number of elements of t outside keep_ranges ([a, b) element ranges) that differ from
    the sentinel.  Counted on the device in slices of at most SLICE_BYTES; one number comes
    back."""
    import torch
    s = _sentinel(t.dtype, sentinel)
    step = SLICE_BYTES // t.element_size()
    total = torch.zeros((), dtype=torch.int64, device=t.device)
    pos = 0
    for a, b in merged(keep_ranges) + [(t.numel(), t.numel())]:
        for lo in range(pos, min(a, t.numel()), step):  # the gap before this kept range
            total += torch.count_nonzero(t[lo:min(lo + step, a)] != s)
        pos = max(pos, b)
    return int(total.item())


# ------------------------------------------------------------------------------- the case table
# What test_gpu_high_offsets.py runs: name -> dict(place: the PLACEMENTS key of the symbol arena
# (dec_place: of the decode launch's, where that is another), enc / dec: the mode of the encode /
# decode launch's symbol arena, slots: the mode of the encoder slots, seed: of the chunks and the
# code layout, peak: every arena the test holds at its peak, as (PLACEMENTS key or a size in
# bytes, how many), for the memory sum).  Slots and code are "u8" arenas.
def _case(place, enc="straddle", dec="exact", slots="exact", peak=None, seed=1, dec_place=None):
    return dict(place=place, dec_place=dec_place or place, enc=enc, dec=dec, slots=slots,
                seed=seed, peak=peak or [(place, 1), ("u8", 1)])


CASES = {
    # 8-bit static coders, one per kernel class
    "static_zipf": _case("u8", seed=1),
    "static_uniform": _case("u8", enc="exact", dec="straddle", slots="straddle", seed=2),
    "static_total_2p20": _case("u8", seed=3),
    "static_direct_table": _case("u8", enc="exact", dec="straddle", slots="straddle", seed=4),
    "adaptive_256": _case("u8", seed=5),
    "adaptive_128": _case("u8", enc="exact", dec="straddle", slots="straddle", seed=6),
    # idx is a second arena indexed like the symbols
    "indexed_k8": _case("u8", peak=[("u8", 3)], seed=7),
    "order1": _case("u8", seed=8),
    "order1_periodic_p4": _case("u8", enc="exact", dec="straddle", slots="straddle", seed=9),
    "order1_lagged_p4_d4": _case("u8", seed=10),
    "wide_1024": _case("u16", seed=11),
    "wide16_65536": _case("u16", enc="exact", dec="straddle", slots="straddle", seed=12),
    "wide16_fine_2p20": _case("u16", seed=13),
    "wide16_65536_index": _case("u16_index", seed=14),
    "chunk_set_k8": _case("u8", enc="exact", dec="straddle", slots="straddle", seed=15),
    "too_long_wide16": _case("u16", seed=16),
    "too_long_wide16_fine": _case("u16", seed=17),
    "too_long_chunk_set": _case("u8", seed=18),
    "too_long_periodic": _case("u8", seed=19),
    "too_long_lagged": _case("u8", seed=20),
    "checksum_u8": _case("u8", peak=[("u8", 1)], seed=21),
    "checksum_u16": _case("u16", enc="exact", peak=[("u16", 1)], seed=22),
    "checksum_u16_index": _case("u16_index", peak=[("u16_index", 1)], seed=23),
    "histograms_u8": _case("u8", peak=[("u8", 1)], seed=24),
    "histograms_u8_exact": _case("u8", enc="exact", peak=[("u8", 1)], seed=25),
    "histograms_u16": _case("u16", peak=[("u16", 1)], seed=26),
    "ideal_bits_order1": _case("u8", peak=[("u8", 1)], seed=27),
    # the triples (12 bytes each) and the slots; then the code and the decoded symbols
    "stream_triples": _case("triples", dec_place="u8", seed=28),
    # row_of (4 bytes per symbol), the symbols indexed like it (1 GiB) and the slots or the code
    "stream_rows": _case("row_of", peak=[("row_of", 1), (1 << 30, 1), ("u8", 1)], seed=29),
    # the slots with the filler (4 GiB) and the container made from them (4 GiB)
    "container_rcb1": _case("u8", peak=[("u8", 2)], seed=30),
    "container_rcb2_checksums": _case("u8", peak=[("u8", 2)], seed=31),
}

# The launch of 2^22 + 64 chunks whose per-chunk histogram rows pass 2^32 bytes: the rows
# buffer (4 GiB and 64 KiB) and a few KiB of symbols.
ROWS_CHUNKS = (1 << 22) + 64
ROWS_REAL = 64            # the real chunks, at the end
ROWS_SAMPLE = 4096        # empty chunks whose rows are compared


def case_lens(name):
    return chunk_lens(CASES[name]["seed"])


def case_layout(name, which, lens=None):
    """The symbol-arena offsets of a case's encode ("enc") or decode ("dec") launch."""
    c = CASES[name]
    eb, boundary, _ = PLACEMENTS[c["place" if which == "enc" else "dec_place"]]
    return layout(case_lens(name) if lens is None else lens, eb, boundary, mode=c[which])


def arena_bytes(place):
    """Bytes of an arena at a placement (or of an arena given by its size): its layouts end
    within 2^18 elements of the boundary (about 40 chunks of at most 300 symbols, or their
    slots), then the tail."""
    if isinstance(place, int):
        return place + (1 << 20)
    eb, boundary, _ = PLACEMENTS[place]
    return arena_elems(boundary // eb + (1 << 18), eb) * eb


def place_elems(place, last_elem=0):
    """Elements of an arena at a placement: one size per placement, whatever the layout, so that
    an arena a test has dropped serves the next one of its kind without a new allocation.
    last_elem: the end of the layout it must hold, with the tail."""
    eb = PLACEMENTS[place][0]
    n = arena_bytes(place) // eb
    assert arena_elems(last_elem, eb) <= n, (place, last_elem)
    return n


def peak_bytes(name):
    return sum(arena_bytes(p) * k for p, k in CASES[name]["peak"])
