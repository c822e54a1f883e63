"""GPU tests of the RCB2 container (include/range_coder.h): the checksum kernel against the numpy
definition (tests/container2_ref.py) over lengths, alignments and launch shapes; containers of
all four kinds byte for byte against the reference framing of the CPU references' streams; round
trips through compress / decompress; the order-1 container's size against the ideal code
lengths; a golden blob; and what a damaged or malformed container raises."""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import range_coder_rust_amd as rc  # noqa: E402
from range_coder_rust_amd import _native as N  # noqa: E402
from range_coder_rust_amd import container as C  # noqa: E402
from range_coder_rust_amd import synth  # noqa: E402
from range_coder_rust_amd.api import _ptr  # noqa: E402
from oracle import container as OC  # noqa: E402
from oracle import cpu  # noqa: E402
from oracle import model_build as O  # noqa: E402
import container2_ref as R  # noqa: E402
import order1_fit_ref as FIT  # noqa: E402
import order1_ref as O1  # noqa: E402
import wide_ref as W  # noqa: E402
from gpu_helpers import dev  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rcb2_order1.json")


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return rc.default_context(0)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def dev16(a):
    """uint16 values as an int16 tensor (the bits are the symbols)."""
    return dev(np.ascontiguousarray(a, np.uint16).view(np.int16))


def np16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


# ---------------------------------------------------------------- the checksum kernel

LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 20001]


def mixed_layout(starts):
    """Chunk offsets (in symbols) in which every length of LENGTHS begins at every start offset
    of `starts` modulo len(starts): a filler chunk before each moves the position there.  The
    fillers are chunks of the launch like the others."""
    m = len(starts)
    off = [0]
    for ln in LENGTHS:
        for a in starts:
            off.append(off[-1] + (a - off[-1]) % m)  # the filler (possibly empty)
            off.append(off[-1] + ln)
    return np.array(off, np.int64)


def check_sums(data, off, sym_bytes, got):
    raw = data.view(np.uint8)
    for k in range(len(off) - 1):
        want = R.checksum(raw[off[k] * sym_bytes:off[k + 1] * sym_bytes])
        assert int(got[k]) == want, (k, int(off[k]), int(off[k + 1] - off[k]))


def test_checksum_u8_every_length_at_every_alignment(ctx):
    off = mixed_layout(range(16))
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    t = dev(data)
    assert t.data_ptr() % 16 == 0 and t.numel() == off[-1]  # (ends with the last chunk's byte)
    got = u32(rc.checksum_batch(t, dev(off)))
    assert len(got) == 2 * len(LENGTHS) * 16
    check_sums(data, off, 1, got)
    # every (length, alignment) pair was a chunk of the launch
    seen = {(int(off[k + 1] - off[k]), int(off[k]) % 16) for k in range(1, len(off) - 1, 2)}
    assert seen == {(ln, a) for ln in LENGTHS for a in range(16)}


def test_checksum_u16_every_length_at_every_symbol_offset(ctx):
    off = mixed_layout(range(8))
    rng = np.random.default_rng(2)
    data = rng.integers(0, 65536, int(off[-1])).astype(np.uint16)
    t = dev16(data)
    assert t.data_ptr() % 16 == 0
    got = u32(rc.checksum_batch(t, dev(off)))
    check_sums(data, off, 2, got)
    if hasattr(torch, "uint16"):  # uint16 tensors, where this torch has them, are the native form
        assert np.array_equal(u32(rc.checksum_batch(t.view(torch.uint16), dev(off))), got)


def test_checksum_grid_stride_rounds(ctx):
    """300 chunks on a grid of 2 workgroups (8 waves): 38 grid-stride rounds, and the same sums
    as the default launch shape gives."""
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 700, 300)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    data = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    t, o = dev(data), dev(off)
    sums = torch.zeros(300, dtype=torch.int32, device="cuda")
    ctx.bind_stream()
    N.check(ctx._lib.rc_checksum_batch_grid_(ctx.handle, _ptr(t), _ptr(o), 300, 1, _ptr(sums), 2),
            "rc_checksum_batch_grid_")
    check_sums(data, off, 1, u32(sums))
    assert np.array_equal(u32(rc.checksum_batch(t, o)), u32(sums))


def test_checksum_of_no_chunks_and_bad_arguments(ctx):
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    assert rc.checksum_batch(empty, dev(np.zeros(1, np.int64))).numel() == 0
    t, o = dev(np.arange(16, dtype=np.uint8)), dev(np.array([0, 16], np.int64))
    s = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib = ctx._lib
    assert lib.rc_checksum_batch(ctx.handle, _ptr(t), _ptr(o), 1, 3, _ptr(s)) == N.RC_E_ARG
    assert lib.rc_checksum_batch(ctx.handle, None, _ptr(o), 1, 1, _ptr(s)) == N.RC_E_ARG
    assert lib.rc_checksum_batch(ctx.handle, _ptr(t), _ptr(o), 1, 1, None) == N.RC_E_ARG


def test_checksum_last_chunk_ends_the_allocation(ctx):
    """The last chunk ends at the last byte of an exactly sized tensor, at a length that is no
    multiple of 16 and from a start that is not 16-B aligned."""
    off = np.array([0, 5, 5 + 5003], np.int64)
    rng = np.random.default_rng(4)
    data = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    t = torch.empty(int(off[-1]), dtype=torch.uint8, device="cuda")
    t.copy_(torch.from_numpy(data))
    check_sums(data, off, 1, u32(rc.checksum_batch(t, dev(off))))


# ---------------------------------------------------------------- containers, byte for byte

SHAPES = [(16, 16), (10000, 3000), (3 * 4096 + 5, 4096)]


def split(data, chunk):
    return [data[i:i + chunk] for i in range(0, len(data), chunk)]


def zipf_data(n, seed):
    c, _, _ = synth.zipf_table()
    rng = np.random.default_rng(seed)
    return rng.choice(256, n, p=np.asarray(c, float) / np.sum(c)).astype(np.uint8)


_cache = {}


def order1_case(K, n):
    """(rows, ctx_map, first_row, data) of a K-row set over 256 symbols and n symbols of its
    chain (made once per (K, n))."""
    if (K, n) not in _cache:
        rng = np.random.default_rng(100 * K + n)
        rows = O1.markov_rows(rng, K, 256, 65536)
        cm = ((np.arange(256) * K) >> 8).astype(np.uint8)
        first = K - 1
        _cache[K, n] = (rows, cm, first, O1.draw_markov(rng, rows, cm, first, n))
    return _cache[K, n]


def wide_case(n):
    if ("w", n) not in _cache:
        rng = np.random.default_rng(n)
        w = rng.pareto(1.1, 4096) + 0.01
        c = 1 + rng.multinomial(65536 - 4096, w / w.sum())
        data = rng.choice(4096, n, p=c / 65536.0).astype(np.uint16)
        data[:2] = (4095, 0)  # both ends of the alphabet occur
        _cache["w", n] = (c, data)
    return _cache["w", n]


def gpu_container(model, data_t, chunk, checksums, encode):
    """Encode on the GPU and pack as RCB2 through the package's pack()."""
    n_sym = data_t.numel()
    n = (n_sym + chunk - 1) // chunk
    sym_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * chunk
    sym_off[-1] = n_sym
    cap = rc.slot_capacity(chunk, 16.0)
    slot_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * cap
    slots = torch.empty(max(n * cap, 16), dtype=torch.uint8, device="cuda")
    out_len, flags = encode(model, data_t, sym_off, slots, slot_off)
    assert int(flags.abs().sum()) == 0
    sums = rc.checksum_batch(data_t, sym_off) if checksums else None
    return C.pack(model, slots, slot_off, out_len, sym_off, sums=sums, rcb2=True)


def check_container(blob, want, data_t):
    got = bytes(blob.cpu().numpy())
    assert len(got) == len(want)
    assert got == want
    out = rc.decompress(blob)
    if data_t.dtype == torch.uint8:
        assert out.dtype == torch.uint8 and torch.equal(out, data_t)
    else:
        assert np.array_equal(np16(out), np16(data_t))


@pytest.mark.parametrize("checksums", [False, True])
@pytest.mark.parametrize("n,chunk", SHAPES)
def test_static_container_bytes(ctx, n, chunk, checksums):
    c, cum, total = synth.zipf_table()
    data = zipf_data(n, n)
    chunks = split(data, chunk)
    codes = []
    for ch in chunks:
        f, b, _ = cpu.encode(c, cum, total, bytes(ch))
        assert f == 0
        codes.append(b)
    want = R.build(R.KIND_STATIC, 256, chunks, codes, c=c, total=total, checksums=checksums)
    m = rc.StaticModel(c, cum, total)
    check_container(gpu_container(m, dev(data), chunk, checksums, rc.encode_batch), want,
                    dev(data))
    if checksums:  # compress() writes the same container
        assert bytes(rc.compress(dev(data), chunk_size=chunk, model=m,
                                 checksum=True).cpu().numpy()) == want


@pytest.mark.parametrize("checksums", [False, True])
@pytest.mark.parametrize("n,chunk", SHAPES)
def test_adaptive_container_bytes(ctx, n, chunk, checksums):
    data = zipf_data(n, n + 1)
    chunks = split(data, chunk)
    codes = []
    for ch in chunks:
        f, b, _ = cpu.encode_adaptive(256, 32, 57343, 256, bytes(ch))
        assert f == 0
        codes.append(b)
    want = R.build(R.KIND_ADAPTIVE, 256, chunks, codes, adaptive=(32, 57343, 256),
                   checksums=checksums)
    m = rc.AdaptiveModel(256, **rc.ADAPTIVE_DEFAULTS)
    check_container(gpu_container(m, dev(data), chunk, checksums, rc.encode_batch), want,
                    dev(data))


@pytest.mark.parametrize("checksums", [False, True])
@pytest.mark.parametrize("K,n,chunk", [(8,) + s for s in SHAPES] + [(1, 10000, 3000),
                                                                    (64, 10000, 3000)])
def test_order1_container_bytes(ctx, K, n, chunk, checksums):
    rows, cm, first, data = order1_case(K, n)
    c, cum = O1.tables(rows)
    chunks = split(data, chunk)
    codes = []
    for ch in chunks:
        f, b = O1.encode_ref(c, cum, 65536, cm, first, ch)
        assert f == 0
        codes.append(b)
    want = R.build(R.KIND_ORDER1, 256, chunks, codes, c=c, total=65536, ctx_map=cm,
                   first_row=first, checksums=checksums)
    m = rc.Order1ModelSet(c, cum, 65536, ctx_map=cm, first_row=first)
    check_container(gpu_container(m, dev(data), chunk, checksums, rc.encode_batch_order1), want,
                    dev(data))
    assert bytes(rc.compress(dev(data), chunk_size=chunk, model=m,
                             checksum=checksums).cpu().numpy()) == want
    # the model read back is the model written
    got = C.model_of(dev(np.array(np.frombuffer(want, np.uint8))))
    assert np.array_equal(got.c, c) and np.array_equal(got.ctx_map, cm)
    assert (got.n_models, got.first_row, got.total) == (K, first, 65536)


@pytest.mark.parametrize("checksums", [False, True])
@pytest.mark.parametrize("n,chunk", SHAPES)
def test_wide_container_bytes(ctx, n, chunk, checksums):
    cf, data = wide_case(n)
    c, cum, total = W.table(cf)
    assert len(c) == 4096 and total == 65536
    chunks = split(data, chunk)
    codes = []
    for ch in chunks:
        f, b = W.encode_ref(c, cum, total, ch)
        assert f == 0
        codes.append(b)
    want = R.build(R.KIND_WIDE, 4096, chunks, codes, c=c, total=total, checksums=checksums)
    m = rc.WideStaticModel(c, cum, total)
    t = dev16(data)
    check_container(gpu_container(m, t, chunk, checksums, rc.encode_batch_wide), want, t)
    assert bytes(rc.compress(t, chunk_size=chunk, model=m,
                             checksum=checksums).cpu().numpy()) == want


# ---------------------------------------------------------------- round trips

def markov_data(n_chunks=16, L=4096, seed=1):
    return np.concatenate(FIT.markov_chunks(8, n_chunks, L, seed))


@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("what", ["markov", "all_equal", "single", "empty"])
def test_order1_round_trip(ctx, what, checksum):
    data = {"markov": lambda: markov_data(),
            "all_equal": lambda: np.full(20000, 7, np.uint8),
            "single": lambda: np.array([200], np.uint8),
            "empty": lambda: np.zeros(0, np.uint8)}[what]()
    x = dev(data) if len(data) else torch.empty(0, dtype=torch.uint8, device="cuda")
    blob = rc.compress(x, chunk_size=4096, order=1, checksum=checksum)
    inf = C.info(blob)
    assert isinstance(inf, N.Container2Info) and blob.numel() == inf.container_bytes
    # empty input has nothing to fit: the order-0 table, as the order-0 path writes it
    assert inf.kind == (0 if what == "empty" else 2)
    assert bool(inf.flags & 1) == checksum and inf.n_syms == len(data)
    if inf.kind == 2:
        assert 1 <= inf.n_models <= 8
    out = rc.decompress(blob)
    assert out.dtype == torch.uint8 and out.numel() == len(data) and torch.equal(out, x)


@pytest.mark.parametrize("checksum", [False, True])
def test_wide_round_trip(ctx, checksum):
    rng = np.random.default_rng(9)
    data = np.minimum(rng.geometric(0.01, 30001) - 1, 2999).astype(np.uint16)
    x = dev16(data)
    blob = rc.compress(x, chunk_size=4096, checksum=checksum)
    inf = C.info(blob)
    assert (inf.kind, inf.sym_bytes, inf.n_symbols) == (3, 2, int(data.max()) + 1)
    out = rc.decompress(blob)
    assert out.dtype == getattr(torch, "uint16", torch.int16)
    assert np.array_equal(np16(out), data)
    # n_symbols from the argument
    inf = C.info(rc.compress(x, chunk_size=4096, n_symbols=4096))
    assert inf.n_symbols == 4096
    with pytest.raises(ValueError):
        rc.compress(x, chunk_size=4096, n_symbols=100)
    with pytest.raises(ValueError):
        rc.compress(x, order=1)


def test_default_compress_is_still_rcb1(ctx):
    """compress(x) with default arguments: the RCB1 bytes of oracle/container.py, as before."""
    data = zipf_data(300000, 77)
    blob = rc.compress(dev(data))
    c, cum, total = O.quantize_counts(np.bincount(data, minlength=256), 1 << 16, O.Q_ALL_SYMBOLS)
    assert bytes(blob.cpu().numpy()) == OC.compress_static(c, cum, total, data, 65536)
    assert isinstance(C.info(blob), N.ContainerInfo) and not isinstance(C.info(blob),
                                                                        N.Container2Info)
    m = rc.AdaptiveModel(256, **rc.ADAPTIVE_DEFAULTS)
    assert bytes(rc.compress(dev(data[:5000]), model=m)[:4].cpu().numpy()) == b"RCB1"


# ---------------------------------------------------------------- compression ratio

def test_order1_container_is_smaller_and_near_its_ideal(ctx):
    """2^18 symbols of the K = 8 Markov source with rotated Zipf rows, 64 chunks
    of 4096.  Both ideals are computed here, from the very models the containers hold, so
    quantisation costs nothing against them; what the payload adds is the stream ends: at most 8
    bytes of flush and 15 of padding per chunk, 64 * 23 * 8 = 11,776 bits, under 1% of the
    smaller ideal (about 1.4e6 bits), and the coder's own 0.04% (§9.4).  2% bounds both."""
    data = markov_data(64, 4096, seed=18)
    assert len(data) == 1 << 18
    x = dev(data)
    sym_off = torch.arange(65, dtype=torch.int64, device="cuda") * 4096
    b0 = rc.compress(x, chunk_size=4096)
    b1 = rc.compress(x, chunk_size=4096, order=1, n_models=8)
    i0, i1 = C.info(b0), C.info(b1)
    _, rows = rc.histogram(x, sym_off, per_chunk=True)
    ideal0 = float(rc.ideal_bits(C.model_of(b0), rows).sum())
    ideal1 = float(rc.ideal_bits_order1(C.model_of(b1), x, sym_off).sum())
    print(f"container bytes: order 0 {b0.numel()}, order 1 {b1.numel()}; payload bits "
          f"{8 * i0.payload_bytes} / {8 * i1.payload_bytes}; ideal bits {ideal0:.0f} / "
          f"{ideal1:.0f}")
    assert np.isfinite(ideal0) and np.isfinite(ideal1) and 0 < ideal1 < ideal0
    assert b1.numel() < b0.numel()
    for inf, ideal in ((i0, ideal0), (i1, ideal1)):
        assert ideal <= 8 * inf.payload_bytes <= 1.02 * ideal
    assert i1.payload_bytes / i0.payload_bytes <= 1.02 * ideal1 / ideal0
    assert torch.equal(rc.decompress(b1), x)


# ---------------------------------------------------------------- golden fixture

def test_golden_container_decodes_to_its_symbols(ctx):
    """A committed kind-2 container with checksums (tests/golden/make_rcb2_fixture.py): the
    format, pinned across commits."""
    g = json.load(open(GOLDEN))
    blob = bytes.fromhex(g["container_hex"])
    syms = np.array(np.frombuffer(bytes.fromhex(g["symbols_hex"]), np.uint8))
    t = dev(np.array(np.frombuffer(blob, np.uint8)))
    inf = C.info(t)
    assert (inf.kind, inf.n_models, inf.flags, inf.n_chunks) == (2, g["n_models"], 1,
                                                                g["n_chunks"])
    assert inf.container_bytes == len(blob)
    assert np.array_equal(rc.decompress(t).cpu().numpy(), syms)
    # and the GPU writes the same bytes from the same model and symbols
    p = R.parse(blob)
    c, cum = O1.tables(p["c"])
    m = rc.Order1ModelSet(c, cum, p["total_freq"], ctx_map=p["ctx_map"], first_row=p["first_row"])
    again = rc.compress(dev(syms), chunk_size=g["chunk_size"], model=m, checksum=True)
    assert bytes(again.cpu().numpy()) == blob


# ---------------------------------------------------------------- corruption

CORRUPT_SEED, CORRUPT_CHUNK, CORRUPT_BYTE, CORRUPT_XOR = 2024, 1, 452, 0x80


def corrupt_case():
    rng = np.random.default_rng(CORRUPT_SEED)
    rows = O1.markov_rows(rng, 8, 256, 65536)
    cm = ((np.arange(256) * 8) >> 8).astype(np.uint8)
    c, cum = O1.tables(rows)
    chunks = [O1.draw_markov(rng, rows, cm, 0, 600) for _ in range(3)]
    return c, cum, cm, chunks


@pytest.mark.parametrize("checksum", [True, False])
def test_flipped_payload_byte(ctx, checksum):
    """One flipped payload byte that the CPU reference decodes WITHOUT a flag to other symbols:
    the silent case that RCB1 lets through.  With checksums decompress must raise; without them
    it returns wrong symbols (or raises), which is the difference the section makes."""
    c, cum, cm, chunks = corrupt_case()
    data = np.concatenate(chunks)
    m = rc.Order1ModelSet(c, cum, 65536, ctx_map=cm, first_row=0)
    blob = rc.compress(dev(data), chunk_size=600, model=m, checksum=checksum)
    assert torch.equal(rc.decompress(blob), dev(data))
    p = R.parse(blob.cpu().numpy())
    count, code = p["chunks"][CORRUPT_CHUNK]
    assert count == 600 and CORRUPT_BYTE < len(code)
    hit = bytearray(code)
    hit[CORRUPT_BYTE] ^= CORRUPT_XOR
    f, out = O1.decode_ref(c, cum, 65536, cm, 0, bytes(hit), 600)
    assert f == 0 and len(out) == 600 and not np.array_equal(out, chunks[CORRUPT_CHUNK])
    pos = p["payload_off"] + sum(R.pad16(len(cd)) for _, cd in p["chunks"][:CORRUPT_CHUNK]) + \
        CORRUPT_BYTE
    bad = blob.clone()
    bad[pos] ^= CORRUPT_XOR
    if checksum:
        # ChecksumError, or the decoder's own flag error: never a return
        with pytest.raises(rc.RangeCoderError) as e:
            rc.decompress(bad)
        if isinstance(e.value, rc.ChecksumError):
            assert e.value.chunk == CORRUPT_CHUNK
    else:
        try:
            got = rc.decompress(bad)
        except rc.RangeCoderError:
            got = None
        assert got is None or not torch.equal(got, dev(data))


# ---------------------------------------------------------------- malformed containers, bad arguments

@pytest.fixture(scope="module")
def good(ctx):
    rows, cm, first, data = order1_case(8, 10000)
    c, cum = O1.tables(rows)
    m = rc.Order1ModelSet(c, cum, 65536, ctx_map=cm, first_row=first)
    blob = rc.compress(dev(data), chunk_size=3000, model=m, checksum=True)
    return blob, C.info(blob), dev(data)


def test_flipped_stored_checksum_names_its_chunk(good):
    blob, inf, data = good
    assert torch.equal(rc.decompress(blob), data)
    for k in (2, 0, 3):
        bad = blob.clone()
        bad[inf.sum_off + 4 * k + 1] ^= 0x04
        with pytest.raises(rc.ChecksumError) as e:
            rc.decompress(bad)
        assert e.value.chunk == k and f"chunk {k}" in str(e.value)
    bad = blob.clone()  # two bad chunks: the lowest is named
    bad[inf.sum_off + 4 * 3] ^= 1
    bad[inf.sum_off + 4 * 1] ^= 1
    with pytest.raises(rc.ChecksumError) as e:
        rc.decompress(bad)
    assert e.value.chunk == 1
    assert issubclass(rc.ChecksumError, rc.RangeCoderError)


def test_malformed_containers_raise_container_error(good):
    blob, inf, _ = good
    bad = blob.clone()  # a table row that no longer sums to the total
    bad[inf.table_off + 4 * 256 * 3] = (int(bad[inf.table_off + 4 * 256 * 3]) + 1) & 255
    with pytest.raises(rc.ContainerError):
        rc.decompress(bad)
    bad = blob.clone()  # a map entry >= K
    bad[inf.table_off + 4 * 256 * 8 + 17] = 8
    with pytest.raises(rc.ContainerError):
        rc.decompress(bad)
    with pytest.raises(rc.ContainerError):  # truncated
        rc.decompress(blob[:-16].clone())
    with pytest.raises(rc.ContainerError):  # truncated inside the table section
        rc.decompress(blob[:1000].clone())
    bad = blob.clone()  # a code length that no longer adds up to the payload
    bad[inf.index_off + 8] = (int(bad[inf.index_off + 8]) + 16) & 255
    with pytest.raises(rc.ContainerError):
        rc.decompress(bad)
    bad = blob.clone()  # a symbol count that no longer adds up
    bad[inf.index_off] = (int(bad[inf.index_off]) + 1) & 255
    with pytest.raises(rc.ContainerError):
        rc.decompress(bad)
    bad = blob.clone()  # unknown flag bits
    bad[56] = 3
    with pytest.raises(rc.ContainerError):
        rc.decompress(bad)
    bad = blob.clone()  # first_row >= K
    bad[24] = 8
    with pytest.raises(rc.ContainerError):
        rc.decompress(bad)


def test_pack_refuses_a_static_set_and_checks_capacity(ctx, good):
    c, cum, total = synth.zipf_table()
    s = rc.StaticModelSet([c, c], [cum, cum], total)
    slots = torch.zeros(64, dtype=torch.uint8, device="cuda")
    off = dev(np.array([0, 64], np.int64))
    ln = dev(np.array([16], np.int64))
    size = ctypes.c_uint64()
    lib = ctx._lib
    assert lib.rc_container2_pack(ctx.handle, s.handle, _ptr(slots), _ptr(off), _ptr(ln),
                                  _ptr(off), 1, None, None, 0,
                                  ctypes.byref(size)) == N.RC_E_ARG
    # the size query and the capacity protocol of rc_container_pack
    m = rc.StaticModel(c, cum, total)
    args = (ctx.handle, m.handle, _ptr(slots), _ptr(off), _ptr(ln), _ptr(off), 1, None)
    assert lib.rc_container2_pack(*args, None, 0, ctypes.byref(size)) == N.RC_E_CAPACITY
    assert size.value == 64 + 1024 + 16 + 16
    dst = torch.full((size.value + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    assert lib.rc_container2_pack(*args, _ptr(dst), size.value - 1,
                                  ctypes.byref(size)) == N.RC_E_CAPACITY
    assert (dst == 0xEE).all()
    assert lib.rc_container2_pack(*args, _ptr(dst), size.value, ctypes.byref(size)) == N.RC_OK
    assert (dst[size.value:] == 0xEE).all() and bytes(dst[:4].cpu().numpy()) == b"RCB2"
    # an RCB1 info is not an RCB2 info
    blob, _, _ = good
    v1 = N.ContainerInfo()
    buf = (ctypes.c_uint8 * ctypes.sizeof(N.Container2Info))()
    ctypes.memmove(buf, ctypes.byref(v1), ctypes.sizeof(v1))
    assert lib.rc_container2_offsets(ctx.handle, _ptr(blob),
                                     ctypes.cast(buf, ctypes.POINTER(N.Container2Info)),
                                     None, None, None) == N.RC_E_ARG
