"""The library's transcript objects (h2g_transcript_*; host only, no device) against the
oracle's Blake2bRead / Keccak256Read (oracle/py/verifier.py): a write-mode sequence of points,
scalars and squeezes gives the bytes and the challenges the oracle gets replaying them, read
mode mirrors it, common_* moves the challenges and not the bytes, and every refused call
(H2G_ERR_ARG) leaves the state as it was."""
import numpy as np
import pytest

import bn254_ref as B
import h2g
import verifier as V

KINDS = ("blake2b", "keccak256")
ERR_ARG, ERR_HANDLE = 1, 5


def fr(x):
    return np.asarray(B.fr_mont_limbs(x % B.R), dtype=np.uint64)


def pt(p):
    return np.asarray(B.g1_affine_mont_limbs(p), dtype=np.uint64)


def fr_int(limbs):
    return B.from_mont(B.from_limbs([int(v) for v in limbs]), B.R)


def pt_ints(limbs):
    return V.affine_from_limbs(limbs)


POINTS = [B.g1_mul(B.G1_GEN, k) for k in (1, 2, 0xDEADBEEF, B.R - 1)]
SCALARS = [0, 1, B.R - 1, 0x1234567890ABCDEF << 100]
# w point, w scalar, q squeeze, c / C common scalar / point
SCRIPT = [("w", 0), ("s", 0), ("q",), ("w", 1), ("w", 2), ("q",), ("q",), ("s", 1), ("C", 3), ("s", 2), ("q",),
          ("c", 3), ("w", 3), ("s", 3), ("q",)]


def err(fn, *args):
    with pytest.raises(h2g.H2GError) as e:
        fn(*args)
    return int(str(e.value).split()[2].rstrip(":"))


def run_write(kind):
    T = h2g.Transcript(kind)
    chal = []
    for op in SCRIPT:
        if op[0] == "w":
            T.write_point(pt(POINTS[op[1]]))
        elif op[0] == "s":
            T.write_scalar(fr(SCALARS[op[1]]))
        elif op[0] == "c":
            T.common_scalar(fr(SCALARS[op[1]]))
        elif op[0] == "C":
            T.common_point(pt(POINTS[op[1]]))
        else:
            chal.append(fr_int(T.squeeze()))
    return T, chal


def replay_oracle(kind, data):
    O = V.TRANSCRIPTS[kind](data)
    chal, vals = [], []
    for op in SCRIPT:
        if op[0] == "w":
            vals.append(O.read_point())
        elif op[0] == "s":
            vals.append(O.read_scalar())
        elif op[0] == "c":
            O.common_scalar(SCALARS[op[1]])
        elif op[0] == "C":
            O.common_point(POINTS[op[1]])
        else:
            chal.append(O.squeeze())
    assert O.pos == len(data)
    return O, chal, vals


@pytest.mark.parametrize("kind", KINDS)
def test_write_mode_matches_the_oracle(kind):
    T, chal = run_write(kind)
    data = T.bytes()
    want = b"".join(B.g1_to_bytes(POINTS[op[1]]) if op[0] == "w" else B.fr_to_repr(SCALARS[op[1]])
                    for op in SCRIPT if op[0] in "ws")
    assert data == want
    _, ochal, vals = replay_oracle(kind, data)
    assert chal == ochal
    assert len(set(chal)) == len(chal)
    assert T.bytes() == data  # finalize leaves the transcript usable
    T.close()


@pytest.mark.parametrize("kind", KINDS)
def test_read_mode_mirrors_it(kind):
    W, chal = run_write(kind)
    data = W.bytes()
    W.close()
    T = h2g.Transcript(kind, proof=data)
    got, vals = [], []
    assert T.remaining() == len(data)
    for op in SCRIPT:
        if op[0] == "w":
            vals.append(pt_ints(T.read_point()))
        elif op[0] == "s":
            vals.append(fr_int(T.read_scalar()))
        elif op[0] == "c":
            T.common_scalar(fr(SCALARS[op[1]]))
        elif op[0] == "C":
            T.common_point(pt(POINTS[op[1]]))
        else:
            got.append(fr_int(T.squeeze()))
    assert got == chal
    assert vals == [POINTS[op[1]] if op[0] == "w" else SCALARS[op[1]] for op in SCRIPT if op[0] in "ws"]
    assert T.remaining() == 0
    T.close()


@pytest.mark.parametrize("kind", KINDS)
def test_common_changes_challenges_not_bytes(kind):
    a, b = h2g.Transcript(kind), h2g.Transcript(kind)
    for T in (a, b):
        T.write_point(pt(POINTS[0]))
    b.common_scalar(fr(7))
    assert a.bytes() == b.bytes()
    ca, cb = fr_int(a.squeeze()), fr_int(b.squeeze())
    assert ca != cb
    O = V.TRANSCRIPTS[kind](a.bytes())
    O.read_point()
    O2 = V.TRANSCRIPTS[kind](a.bytes())
    O2.read_point()
    O2.common_scalar(7)
    assert (ca, cb) == (O.squeeze(), O2.squeeze())
    b.common_point(pt(POINTS[1]))
    O2.common_point(POINTS[1])
    assert a.bytes() == b.bytes() and fr_int(b.squeeze()) == O2.squeeze()
    a.close()
    b.close()


def _no_curve_x():
    x = 1
    while B.fq_sqrt((x * x * x + 3) % B.P) is not None:
        x += 1
    return x


@pytest.mark.parametrize("kind", KINDS)
def test_refused_calls_leave_the_state(kind):
    """each refusal is H2G_ERR_ARG, and the next squeeze equals the oracle's without it"""
    r_limbs = np.asarray(B.to_limbs(B.R), dtype=np.uint64)  # r itself, as raw limbs: >= r
    x_ge_p = np.concatenate([np.asarray(B.to_limbs(B.P), dtype=np.uint64), pt(POINTS[0])[4:]])
    off_curve = pt(POINTS[0]).copy()
    off_curve[4:] = pt(POINTS[1])[4:]
    T = h2g.Transcript(kind)
    T.write_point(pt(POINTS[2]))
    O = V.TRANSCRIPTS[kind](B.g1_to_bytes(POINTS[2]))
    O.read_point()
    zero_pt = np.zeros(8, dtype=np.uint64)
    for fn, arg in ((T.write_point, zero_pt), (T.common_point, zero_pt), (T.write_scalar, r_limbs),
                    (T.common_scalar, r_limbs), (T.write_point, x_ge_p), (T.write_point, off_curve)):
        assert err(fn, arg) == ERR_ARG
    assert err(T.read_point) == ERR_ARG and err(T.read_scalar) == ERR_ARG and err(T.remaining) == ERR_ARG  # wrong mode
    assert T.bytes() == B.g1_to_bytes(POINTS[2])
    assert fr_int(T.squeeze()) == O.squeeze()
    T.close()

    # read mode: a scalar >= r, x >= p, an x with no curve point, the identity, a read past the end
    good = B.g1_to_bytes(POINTS[1])
    bad = [B.R.to_bytes(32, "little"), B.P.to_bytes(32, "little"), _no_curve_x().to_bytes(32, "little"), bytes(32)]
    for i, enc in enumerate(bad):
        T = h2g.Transcript(kind, proof=good + enc)
        O = V.TRANSCRIPTS[kind](good)
        assert pt_ints(T.read_point()) == O.read_point()
        assert err(T.read_scalar if i == 0 else T.read_point) == ERR_ARG
        assert T.remaining() == 32
        assert err(T.write_point, pt(POINTS[0])) == ERR_ARG and err(T.write_scalar, fr(1)) == ERR_ARG  # wrong mode
        assert err(T.bytes) == ERR_ARG
        assert fr_int(T.squeeze()) == O.squeeze()
        T.close()
    T = h2g.Transcript(kind, proof=good + bytes(31))
    O = V.TRANSCRIPTS[kind](good)
    T.read_point(), O.read_point()
    assert err(T.read_point) == ERR_ARG and err(T.read_scalar) == ERR_ARG
    assert T.remaining() == 31 and fr_int(T.squeeze()) == O.squeeze()
    T.close()


def test_handles():
    T = h2g.Transcript("blake2b")
    h = T.handle
    T.close()
    c = np.zeros(4, dtype=np.uint64)
    assert h2g.lib().h2g_transcript_squeeze(h, h2g.p64(c)) == ERR_HANDLE
    assert h2g.lib().h2g_transcript_free(h) == ERR_HANDLE
    t = h2g.U64()
    assert h2g.lib().h2g_transcript_new_write(2, h2g.ctypes.byref(t)) == ERR_ARG
