"""GPU: batched base64 codec (wire.hip) vs the reference's own encoder (Python base64,
messaging.py:607, 829, 852-853).  Bar: byte-exact text and bytes; malformed records flagged
exactly where strict decoding (b64decode(validate=True) + length) rejects them."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 4, 5, 11, 12, 13, 16, 23, 24, 25, 32, 768, 800, 1088, 1184, 1568, 9616, 15744]


@pytest.fixture(scope="module")
def codec():
    from qrkem.wire import Base64Codec
    return Base64Codec(device=0)


@pytest.mark.parametrize("L", LENGTHS)
def test_encode_decode_match_python(codec, L):
    import wire_spec
    rng = np.random.default_rng(L)
    n = 37 if L < 5000 else 5
    data = rng.integers(0, 256, (n, L), dtype=np.uint8)
    txt = codec.encode(torch.from_numpy(data).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(txt.cpu().numpy(), wire_spec.encode_records(data))
    back, st = codec.decode(txt, L)
    torch.cuda.synchronize()
    assert np.array_equal(back.cpu().numpy(), data)
    assert int(st.abs().sum()) == 0


def test_malformed_records_flagged(codec):
    import wire_spec
    rng = np.random.default_rng(3)
    for L in (1, 2, 3, 10, 1184):
        n = 64
        data = rng.integers(0, 256, (n, L), dtype=np.uint8)
        txt = wire_spec.encode_records(data).copy()
        W = txt.shape[1]
        for i in range(1, n, 2):  # corrupt odd records
            kind = (i // 2) % 4
            pos = int(rng.integers(0, W))
            if kind == 0:
                txt[i, pos] = ord("!")
            elif kind == 1:
                txt[i, pos] = 0xC3  # non-ASCII
            elif kind == 2:
                txt[i, min(pos, max(W - 5, 0))] = ord("=")  # padding in the middle
            else:
                txt[i, -1] = ord("A") if txt[i, -1] == ord("=") else ord("=")  # padding count
        out, st = codec.decode(torch.from_numpy(txt).cuda(), L)
        torch.cuda.synchronize()
        st, out = st.cpu().numpy(), out.cpu().numpy()
        for i in range(n):
            want = wire_spec.decode_record(txt[i].tobytes(), L)
            assert (st[i] == 0) == (want is not None), (L, i, txt[i].tobytes()[-8:])
            if want is not None:
                assert out[i].tobytes() == want


def test_large_batch_roundtrip(codec):
    n, L = 1 << 18, 1184
    data = torch.randint(0, 256, (n, L), dtype=torch.uint8, device="cuda")
    txt = codec.encode(data)
    back, st = codec.decode(txt, L)
    torch.cuda.synchronize()
    assert torch.equal(back, data) and int(st.abs().sum()) == 0
    import base64
    idx = [0, 1, n // 2, n - 1]
    h = data[idx].cpu().numpy()
    t = txt[idx].cpu().numpy()
    for a, b in zip(h, t):
        assert base64.b64encode(a.tobytes()) == b.tobytes()


@pytest.mark.parametrize("L", [1, 2, 3, 5])
def test_tight_hipmalloc_buffers(codec, L):
    """records shorter than a 12-byte (16-character) chunk must not be loaded past the
    end of the input.  The input here is a bare hipMalloc of exactly n*L bytes (n*IL characters),
    not a torch tensor whose caching allocator pads the block, so the last records' chunks end at
    the allocation's last byte."""
    import ctypes as ct
    import wire_spec
    from qrkem._native import LIB
    hip = ct.CDLL("libamdhip64.so")
    n = 8191  # odd count: the last record's chunk is not 4-byte aligned for every L
    rng = np.random.default_rng(100 + L)
    data = rng.integers(0, 256, (n, L), dtype=np.uint8)
    want_txt = wire_spec.encode_records(data)
    IL = want_txt.shape[1]
    pin, ptxt = ct.c_void_p(), ct.c_void_p()
    assert hip.hipMalloc(ct.byref(pin), ct.c_size_t(n * L)) == 0
    assert hip.hipMalloc(ct.byref(ptxt), ct.c_size_t(n * IL)) == 0
    try:
        assert hip.hipMemcpy(pin, data.ctypes.data_as(ct.c_void_p), ct.c_size_t(n * L), 1) == 0
        assert hip.hipMemcpy(ptxt, want_txt.ctypes.data_as(ct.c_void_p), ct.c_size_t(n * IL), 1) == 0
        txt = torch.empty((n, IL), dtype=torch.uint8, device="cuda")
        back = torch.empty((n, L), dtype=torch.uint8, device="cuda")
        st = torch.zeros((n,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert LIB.qrk_base64_encode_batch(codec._ctx, n, pin, L, ct.c_void_p(txt.data_ptr()), s) == 0
        assert LIB.qrk_base64_decode_batch(codec._ctx, n, ptxt, L, ct.c_void_p(back.data_ptr()),
                                           ct.c_void_p(st.data_ptr()), s) == 0
        torch.cuda.synchronize()
        assert np.array_equal(txt.cpu().numpy(), want_txt)
        assert np.array_equal(back.cpu().numpy(), data)
        assert int(st.abs().sum()) == 0
    finally:
        hip.hipFree(pin)
        hip.hipFree(ptxt)


# ---------------------------------------------------------------- strictness sweeps
# All three padding counts, one- and two-chunk records (12 bytes / 16 characters a chunk) and a short
# last chunk.  The reference throughout is wire_spec.decode_record (b64decode(validate=True) + length).
STRICT_LENGTHS = [1, 2, 3, 13, 14, 15, 24, 25]
ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"


def _record(L, seed=0):
    """(data uint8 [L], its base64 text uint8 [4 ceil(L/3)])."""
    import wire_spec
    data = np.random.default_rng(1000 * seed + L).integers(0, 256, (1, L), dtype=np.uint8)
    return data[0], wire_spec.encode_records(data)[0]


def _decode(codec, txt, L):
    out, st = codec.decode(torch.from_numpy(np.ascontiguousarray(txt)).cuda(), L)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


def _check_against_spec(out, st, txt, L, what):
    """Status 0 exactly where the spec decodes to L bytes, and then the same bytes; returns the number
    of accepted rows."""
    import wire_spec
    ok = 0
    for i in range(len(txt)):
        want = wire_spec.decode_record(txt[i].tobytes(), L)
        assert st[i] in (0, -1)
        assert (st[i] == 0) == (want is not None), f"L={L} {what(i)}: status {st[i]}, text {txt[i].tobytes()!r}"
        if want is not None:
            assert out[i].tobytes() == want, f"L={L} {what(i)}: bytes differ, text {txt[i].tobytes()!r}"
            ok += 1
    return ok


@pytest.mark.parametrize("L", STRICT_LENGTHS)
def test_every_byte_value_in_every_slot(codec, L):
    """Every byte value 0..255 in each of the four slots of the first group, of the last full group and of
    the final group (its padding positions included), one row per (group, slot, value): the neighbours of
    the alphabet ranges, NUL, newline, 0x7F, 0x80, 0xFF and '=' outside the padding among them."""
    _, t = _record(L)
    W = len(t)
    groups = sorted({0, W // 4 - 1} | ({(L // 3) - 1} if L >= 3 else set()))
    where = [(g, k, v) for g in groups for k in range(4) for v in range(256)]
    txt = np.tile(t, (len(where), 1))
    for i, (g, k, v) in enumerate(where):
        txt[i, 4 * g + k] = v
    out, st = _decode(codec, txt, L)
    ok = _check_against_spec(out, st, txt, L, lambda i: "group %d slot %d value 0x%02X" % where[i])
    # the spec itself: 64 values per data slot, none but '=' per padding slot (fewer where a slot's value
    # changes a canonical-length decode; the count is the reference's, this only shows the sweep bites)
    assert 0 < ok < len(where) and (st == -1).sum() >= len(where) * 3 // 4


@pytest.mark.parametrize("L", [1184, 25])
def test_bad_character_at_every_position(codec, L):
    """'!' at every character position in turn, one row per position, padding positions included: every
    such row is rejected, and the intact rows among them (every fifth row, first and last) are not."""
    data, t = _record(L)
    W = len(t)
    rows, bad_pos = [], []
    for pos in range(W):
        if pos % 4 == 1:
            rows.append(t), bad_pos.append(-1)
        r = t.copy()
        r[pos] = ord("!")
        rows.append(r), bad_pos.append(pos)
    rows, bad_pos = [t] + rows + [t], np.array([-1] + bad_pos + [-1])
    out, st = _decode(codec, np.stack(rows), L)
    missed = bad_pos[(bad_pos >= 0) & (st != -1)]
    assert len(missed) == 0, f"L={L}: '!' accepted at positions {missed[:8]}"
    assert (st[bad_pos < 0] == 0).all(), f"L={L}: intact rows {np.nonzero((bad_pos < 0) & (st != 0))[0][:8]} rejected"
    assert (out[bad_pos < 0] == data).all()
    inner = np.nonzero(bad_pos < 0)[0][1:-1]
    assert len(inner) == W // 4 and (bad_pos[inner - 1] >= 0).all() and (bad_pos[inner + 1] >= 0).all()
    _check_against_spec(out, st, np.stack(rows), L, lambda i: f"row {i}")


@pytest.mark.parametrize("L", [x for x in STRICT_LENGTHS if x % 3])
def test_noncanonical_trailing_bits_are_accepted(codec, L):
    """The last data character of a padded record carries 4 (L = 1 mod 3) or 2 (L = 2 mod 3) bits that no
    byte uses.  Python's strict decoder accepts any value there, so the batched one must: all 16 / 4
    values decode to the record's bytes."""
    import wire_spec
    data, t = _record(L)
    unused = 4 if L % 3 == 1 else 2
    pos = len(t) - 1 - (3 - L % 3)
    assert t[pos + 1] == ord("=") and t[pos] != ord("=")
    base = ALPHABET.index(bytes([t[pos]]))
    assert base & ((1 << unused) - 1) == 0  # the encoder writes zeros
    txt = np.tile(t, (1 << unused, 1))
    for v in range(1 << unused):
        txt[v, pos] = ALPHABET[base | v]
    for r in txt:
        assert wire_spec.decode_record(r.tobytes(), L) == data.tobytes()
    out, st = _decode(codec, txt, L)
    assert (st == 0).all(), f"L={L}: trailing bits {np.nonzero(st)[0]} rejected"
    assert (out == data).all()


@pytest.mark.parametrize("L", [1184, 25])
def test_two_bad_chunks_in_one_record(codec, L):
    """Bad characters in two different 16-character chunks of one record (two lanes flag the same record):
    status -1, the records either side of it 0."""
    data, t = _record(L)
    W = len(t)
    nchunk = (W + 15) // 16
    pairs = [(0, nchunk - 1), (0, 1), (nchunk // 2, nchunk - 1), (nchunk - 2, nchunk - 1)]
    txt = np.tile(t, (2 * len(pairs) + 1, 1))
    for i, (a, b) in enumerate(pairs):
        assert a != b
        txt[2 * i + 1, 16 * a + (5 * i) % 4] = ord("!")
        txt[2 * i + 1, min(16 * b + 3 + i, W - 1)] = 0xC3 if i % 2 else ord("!")
    out, st = _decode(codec, txt, L)
    assert st.tolist() == [0, -1] * len(pairs) + [0]
    assert (out[0::2] == data).all()
    _check_against_spec(out, st, txt, L, lambda i: f"row {i}")
