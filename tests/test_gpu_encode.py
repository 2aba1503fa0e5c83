"""GPU: the TX chain on caller payloads (csrc/encode.hip: pscl_encode_device,
pscl_channel_payload_device and the SCLDecoder tensor methods above them).

Expected message and transmitted bits come from the oracle (attach_crc, polar_transform) and the
host mirrors of the NR interleaver and rate matching (encode_cases.expected), never from the code
under test.  The channel is pinned to the existing one: called with the payloads pscl_channel_device
drew, pscl_channel_payload_device must give that call's message words and float64 rows bit for bit.
Every comparison is on bits (float rows as integer views); the one bound, on a noise term
recomputed from two rows, is derived where it is used.  Outputs land in sentinel-filled buffers with
one guard row behind them."""
import numpy as np
import pytest

import oracle
from encode_cases import CODES, POLY24, RATE_MATCHED, crc_degree, expected, info_set, pack, payloads, unpack
from polar_code_amd import _native

pytestmark = pytest.mark.gpu

EINVAL = _native.PSCL_EINVAL
SENTINEL = 0x5A
BATCHES = (1, 63, 64, 65, 257)  # a partial wavefront, a full one, one lane more, a partial second workgroup
BMAX = max(BATCHES)
U64 = np.uint64

_EXPECTED = {}


def reference(N, K, crc, E=0):
    """(payload bits, payload words with garbage above k_payload, msg bits, transmitted bits) of BMAX
    frames of the code: computed once and shared, read-only."""
    key = (N, K, crc, E)
    if key not in _EXPECTED:
        bits = payloads(N, K, crc, BMAX)
        bits[0], bits[1] = 0, 1
        words = pack(bits)
        kp = bits.shape[1]
        if kp & 63:  # bits at and above k_payload are to be masked off
            words[:, -1] |= U64(0xFFFFFFFFFFFFFFFF) << U64(kp & 63)
        msg, tx = expected(N, K, crc, E, bits)
        for a in (bits, words, msg, tx):
            a.setflags(write=False)
        _EXPECTED[key] = (bits, words, msg, tx)
    return _EXPECTED[key]


class Out:
    """One device output of `rows` rows of `width` items: sentinel-filled, one guard row behind it."""

    def __init__(self, mem, rows, width, dtype):
        self.mem, self.rows, self.width, self.dtype = mem, rows, width, np.dtype(dtype)
        self.nbytes = max((rows + 1) * width * self.dtype.itemsize, 8)
        self.ptr = mem.alloc(self.nbytes)
        mem.memset(self.ptr, SENTINEL, self.nbytes)

    def get(self):
        raw = self.mem.download(self.ptr, self.nbytes, np.uint8)[:(self.rows + 1) * self.width * self.dtype.itemsize]
        guard = raw[self.rows * self.width * self.dtype.itemsize:]
        assert np.all(guard == SENTINEL), "the call wrote past its last row"
        return raw[:self.rows * self.width * self.dtype.itemsize].view(self.dtype).reshape(self.rows, self.width)


def upload(mem, arr):
    d = mem.alloc(max(arr.nbytes, 8))
    mem.upload(d, np.ascontiguousarray(arr))
    return d


def run_encode(dec, words, B, want=("msg", "code", "sym"), f32=False):
    """pscl_encode_device on the first B payloads -> dict of the requested outputs (host arrays)."""
    E = dec.E or dec.N
    with _native.DeviceArena(dec) as mem:
        d_pay = upload(mem, words[:B])
        outs = {}
        if "msg" in want:
            outs["msg"] = Out(mem, B, dec.W, U64)
        if "code" in want:
            outs["code"] = Out(mem, B, dec.code_words, U64)
        if "sym" in want:
            outs["sym"] = Out(mem, B, E, np.float32 if f32 else np.float64)
        dec.encode_device(d_pay, B, d_msg=outs["msg"].ptr if "msg" in outs else 0,
                          d_code=outs["code"].ptr if "code" in outs else 0,
                          d_sym=outs["sym"].ptr if "sym" in outs else 0, sym_f32=f32)
        dec.sync()
        return {k: o.get() for k, o in outs.items()}


def check_outputs(dec, got, B, msg, tx, f32=False):
    K, E = dec.K, dec.E or dec.N
    if "msg" in got:
        np.testing.assert_array_equal(unpack(got["msg"], K), msg[:B])
        if K & 63:
            assert not np.any(got["msg"][:, -1] >> U64(K & 63))
    if "code" in got:
        np.testing.assert_array_equal(unpack(got["code"], E), tx[:B])
        if E & 63:  # bits past E in the last code word are zero
            assert not np.any(got["code"][:, -1] >> U64(E & 63))
    if "sym" in got:
        ft, it = (np.float32, np.uint32) if f32 else (np.float64, np.uint64)
        assert got["sym"].dtype == ft
        np.testing.assert_array_equal(got["sym"].view(it), (1 - 2 * tx[:B].astype(ft)).view(it))


@pytest.mark.parametrize("N,K,crc", CODES)
def test_encode_equals_the_oracle_at_every_batch_size(N, K, crc):
    _, words, msg, tx = reference(N, K, crc)
    dec = _native.Decoder(N, info_set(N, K), 2, crc)
    assert dec.k_payload == K - crc_degree(crc) and dec.payload_words == words.shape[1]
    for B in BATCHES:
        check_outputs(dec, run_encode(dec, words, B), B, msg, tx)
    dec.close()


@pytest.mark.parametrize("N,K,crc,E", RATE_MATCHED + [(32, 20, "0x107", 50)])
def test_rate_matched_encode_equals_interleave_then_rate_match(N, K, crc, E):
    _, words, msg, tx = reference(N, K, crc, E)
    dec = _native.Decoder(N, info_set(N, K), 2, crc)
    dec.set_rate_match(E)
    for B, f32 in ((65, True), (BMAX, False)):
        check_outputs(dec, run_encode(dec, words, B, f32=f32), B, msg, tx, f32=f32)
    dec.set_rate_match(0)  # and off again: the plain codeword
    _, _, msg0, tx0 = reference(N, K, crc)
    check_outputs(dec, run_encode(dec, words, 65), 65, msg0, tx0)
    dec.close()


@pytest.mark.parametrize("N,K,crc,E", [(128, 74, POLY24, 0), (256, 140, POLY24, 0), (128, 88, POLY24, 201), (256, 140, POLY24, 320)])
def test_each_output_alone(N, K, crc, E):
    _, words, msg, tx = reference(N, K, crc, E)
    dec = _native.Decoder(N, info_set(N, K), 2, crc)
    if E:
        dec.set_rate_match(E)
    B = 65
    for want, f32 in ((("msg",), False), (("code",), False), (("sym",), False), (("sym",), True), (("msg", "code", "sym"), True)):
        got = run_encode(dec, words, B, want=want, f32=f32)
        assert sorted(got) == sorted(want)
        check_outputs(dec, got, B, msg, tx, f32=f32)
    dec.close()


# ---- the channel, pinned to pscl_channel_device

def channel_pair(dec, seed, sid, ebno, rate, frame0, B, payload_words=None):
    """(msg words, float64 rows) of pscl_channel_device, and (msg words, float64 rows, float32 rows) of
    pscl_channel_payload_device on that call's payloads (or on payload_words) -- same stream arguments."""
    E, kp = dec.E or dec.N, dec.k_payload
    with _native.DeviceArena(dec) as mem:
        r_llr, r_msg = Out(mem, B, E, np.float64), Out(mem, B, dec.W, U64)
        dec.channel_device(seed, sid, ebno, rate, kp, frame0, B, r_llr.ptr, r_msg.ptr)
        dec.sync()
        ref_msg, ref_llr = r_msg.get(), r_llr.get()
        if payload_words is None:  # the low k_payload bits of the message words
            payload_words = pack(unpack(ref_msg, kp), dec.payload_words)
        d_pay = upload(mem, payload_words)
        llr64, llr32 = Out(mem, B, E, np.float64), Out(mem, B, E, np.float32)
        msg64, msg32 = Out(mem, B, dec.W, U64), Out(mem, B, dec.W, U64)
        dec.channel_payload_device(d_pay, seed, sid, ebno, rate, frame0, B, d_llr=llr64.ptr, d_msg=msg64.ptr)
        dec.channel_payload_device(d_pay, seed, sid, ebno, rate, frame0, B, d_llr=llr32.ptr, llr_f32=True, d_msg=msg32.ptr)
        dec.sync()
        m64, m32 = msg64.get(), msg32.get()
        np.testing.assert_array_equal(m64, m32)
        return ref_msg, ref_llr, m64, llr64.get(), llr32.get()


@pytest.mark.parametrize("N,K,crc,E,ebno,frame0,B", [
    (128, 64, POLY24, 0, 5.0, 123456789, BMAX),
    (128, 88, POLY24, 256, 2.0, 7, BMAX),
    (128, 88, POLY24, 100, 2.0, 7, BMAX),
    (8, 6, "0xB", 0, 3.0, 0, BMAX),
    (256, 140, POLY24, 0, 3.0, 99, BMAX),
    (128, 64, POLY24, 0, 5.0, 2**32 - 100, 300),  # the frame counter crosses 2^32
    (256, 140, POLY24, 320, 3.0, 2**32 - 100, 300),
])
def test_channel_on_the_drawn_payloads_is_bit_identical(N, K, crc, E, ebno, frame0, B):
    dec = _native.Decoder(N, info_set(N, K), 2, crc)
    if E:
        dec.set_rate_match(E)
    rate = dec.k_payload / (E or N)
    ref_msg, ref_llr, msg, llr64, llr32 = channel_pair(dec, 0x1234ABCD5678, 42, ebno, rate, frame0, B)
    np.testing.assert_array_equal(msg, ref_msg)
    np.testing.assert_array_equal(llr64.view(U64), ref_llr.view(U64))
    assert np.all(np.isfinite(ref_llr)) and ref_llr.std() > 0.5  # (rows were drawn at all)
    # float32 rows: the float64 value rounded once
    np.testing.assert_array_equal(llr32.view(np.uint32), ref_llr.astype(np.float32).view(np.uint32))
    dec.close()


def test_another_payload_changes_only_the_signs_the_codeword_difference_implies():
    N, K, crc, ebno, B = 128, 64, POLY24, 5.0, 3
    dec = _native.Decoder(N, info_set(N, K), 2, crc)
    kp, rate = dec.k_payload, dec.k_payload / N
    bits = payloads(N, K, crc, B, seed=5)
    msg_bits, tx = expected(N, K, crc, 0, bits)
    ref_msg, ref_llr, msg, llr, _ = channel_pair(dec, 77, 3, ebno, rate, 1000, B, payload_words=pack(bits))
    np.testing.assert_array_equal(unpack(msg, K), msg_bits)
    ref_tx = expected(N, K, crc, 0, unpack(ref_msg, kp))[1]
    same = tx == ref_tx
    assert 20 < np.count_nonzero(~same[0]) < 108  # (the codewords differ in many places, not in all)
    # where the codeword bits agree the rows agree bit for bit (same symbol, same noise)
    np.testing.assert_array_equal(llr.view(U64)[same], ref_llr.view(U64)[same])
    # elsewhere the noise recomputed from either row is the same.  row = fl(fl(sym + n) s) with
    # s = fl(2 / var): two roundings (2 u, u = 2^-53); a' = row * (var / 2) adds the rounding of var / 2
    # against 1 / s (<= 2 u) and of the product (u), so a' = (sym + n)(1 + d), |d| <= 6 u to first order,
    # and n' = a' - sym adds u |n'|.  The two recomputed noises differ by at most
    # 6 u (|sym + n| + |-sym + n|) + 2 u |n| <= 16 u (1 + |n|).
    var = 1.0 / (2.0 * rate * 10 ** (ebno / 10.0))
    n_ref = ref_llr * (var / 2.0) - (1.0 - 2.0 * ref_tx)
    n_new = llr * (var / 2.0) - (1.0 - 2.0 * tx)
    bound = 16 * 2.0 ** -53 * (1.0 + np.abs(n_ref))
    print("max |noise difference| / bound", float((np.abs(n_new - n_ref) / bound).max()))
    assert np.all(np.abs(n_new - n_ref) <= bound)
    dec.close()


# ---- round trip through the tensor methods

def _words_tensor(torch, words, device):
    return torch.from_numpy(np.array(words, dtype=U64).view(np.int64)).to(device)


@pytest.mark.parametrize("N,K,L", [(128, 64, 8), (256, 140, 4)])
def test_round_trip_encode_tensor_decode_tensor(N, K, L):
    """(128,64) L = 8 takes the native float32 decode, (256,140) L = 4 the widening fallback.  On a
    side stream: the handle runs on the caller's torch stream, the tensors' producer and consumer."""
    import torch

    from polar_code_amd.polar.scl import SCLDecoder

    _, words, msg, tx = reference(N, K, POLY24)
    dec = SCLDecoder(N, info_set(N, K), L, POLY24)
    assert dec.native.f32_available() == (N == 128)
    dev = torch.device("cuda", 0)
    B = 193
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        pw = _words_tensor(torch, words[:B], dev)
        msg_words, code_words, sym = dec.encode_tensor(pw, symbols=torch.float32)
        assert sym.dtype == torch.float32 and tuple(sym.shape) == (B, N) and tuple(msg_words.shape) == (B, dec.native.W)
        best, flags = dec.decode_tensor(sym * 4.0)
        two = dec.encode_tensor(pw)
        sym64 = dec.encode_tensor(pw, symbols=torch.float64)[2]
    stream.synchronize()
    assert len(two) == 2 and torch.equal(two[0], msg_words) and torch.equal(two[1], code_words)
    assert torch.equal(best, msg_words)
    assert bool(torch.all((flags & _native.PSCL_FLAG_CRC_PASS) != 0))
    np.testing.assert_array_equal(unpack(msg_words.cpu().numpy().view(U64), K), msg[:B])
    np.testing.assert_array_equal(unpack(code_words.cpu().numpy().view(U64), N), tx[:B])
    assert sym64.dtype == torch.float64 and torch.equal(sym64, sym.double())
    dec.native.close()


def test_transmit_tensor_float32_rows_decode_as_the_oracle_decodes_them():
    import torch

    from polar_code_amd.polar.scl import SCLDecoder

    N, K, L, B = 128, 64, 8, 257
    _, words, msg, _ = reference(N, K, POLY24)
    info = info_set(N, K)
    dec = SCLDecoder(N, info, L, POLY24)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        pw = _words_tensor(torch, words[:B], dev)
        llr, msg_words = dec.transmit_tensor(pw, 8.0, seed=2024, stream_id=1, frame0=50, dtype=torch.float32)
        assert llr.dtype == torch.float32 and tuple(llr.shape) == (B, N)
        best, flags = dec.decode_tensor(llr)
        # the default: float64 rows at rate k_payload / E, whose float32 rounding is the float32 call's row
        llr64, _ = dec.transmit_tensor(pw, 8.0, seed=2024, stream_id=1, frame0=50)
    stream.synchronize()
    np.testing.assert_array_equal(unpack(msg_words.cpu().numpy().view(U64), K), msg[:B])
    rows = llr.cpu().numpy().astype(np.float64)  # (widening is exact)
    want_bits, want_ok = oracle.decode_batch(rows, info, L, POLY24)
    np.testing.assert_array_equal(unpack(best.cpu().numpy().view(U64), K), want_bits)
    np.testing.assert_array_equal((flags.cpu().numpy() & _native.PSCL_FLAG_CRC_PASS) != 0, want_ok)
    assert want_ok.mean() > 0.9  # (8 dB: the link works)
    assert llr64.dtype == torch.float64 and torch.equal(llr64.float(), llr)
    dec.native.close()


def test_encode_host_arrays():
    from polar_code_amd.polar.scl import SCLDecoder

    N, K, E = 128, 88, 201
    bits, _, msg, tx = reference(N, K, POLY24, E)
    dec = SCLDecoder(N, info_set(N, K), 4, POLY24)
    dec.native.set_rate_match(E)
    out = dec.encode(bits[:70])
    np.testing.assert_array_equal(out["msg"], msg[:70])
    np.testing.assert_array_equal(out["code"], tx[:70])
    cpu = dec.encode(bits[:70], device="cpu")  # the host form gives the same words
    np.testing.assert_array_equal(cpu["msg"], out["msg"])
    np.testing.assert_array_equal(cpu["code"], out["code"])
    dec.native.close()


# ---- refusals

def test_refusals_name_their_reason():
    lib = _native.lib()
    dec = _native.Decoder(128, info_set(128, 64), 2, POLY24)
    h = dec.handle
    with _native.DeviceArena(dec) as mem:
        d_pay, d_out = mem.alloc(64 * 8), mem.alloc(64 * 128 * 8)
        mem.memset(d_pay, 0, 64 * 8)

        def enc(pay=d_pay, B=4, msg=d_out, code=None, sym=None, f32=0):
            return lib.pscl_encode_device(h, pay, B, msg, code, sym, f32)

        def chan(pay=d_pay, rate=0.5, frame0=0, B=4, llr=d_out, f32=0, msg=None):
            return lib.pscl_channel_payload_device(h, pay, 1, 0, 3.0, rate, frame0, B, llr, f32, msg)

        for call, kw, word in ((enc, dict(pay=None), "payload"), (enc, dict(B=-1), "B"), (enc, dict(msg=None), "output"),
                               (enc, dict(f32=2), "dtype"), (enc, dict(f32=-1), "dtype"),
                               (chan, dict(pay=None), "payload"), (chan, dict(B=-1), "B"),
                               (chan, dict(frame0=-1), "frame0"), (chan, dict(llr=None), "output"),
                               (chan, dict(rate=0.0), "rate"), (chan, dict(rate=-1.0), "rate"),
                               (chan, dict(rate=float("nan")), "rate"), (chan, dict(f32=2), "dtype")):
            rc = call(**kw)
            assert rc == EINVAL and word in _native.last_error(), (kw, rc, _native.last_error())
        assert lib.pscl_encode_device(None, d_pay, 4, d_out, None, None, 0) == EINVAL and "handle" in _native.last_error()
        # B = 0 is no error and no launch; a message alone is a valid channel call
        assert enc(B=0) == 0 and chan(B=0) == 0 and chan(llr=None, msg=d_out) == 0
    dec.close()
