"""Host side of bls_mi355x.kzg with no device: the challenge's transcript, install / uninstall on a module-like
object, and the length and range assertions that are decided before any device call (the stub context raises a
RuntimeError on the first one)."""
import hashlib
import types

import pytest

import kzg_inputs as K
from bls_mi355x import kzg

R = K.R
BLOB = bytes(kzg.BYTES_PER_BLOB)
G1 = K.IDENTITY48


class NoDevice:
    """a context whose library must not be reached"""

    h = None

    @property
    def lib(self):
        raise RuntimeError("device call")

    def check(self, rc):
        raise RuntimeError("device call")


@pytest.fixture()
def setup():
    s = kzg.KzgSetup.__new__(kzg.KzgSetup)
    s.ctx, s.table, s.first = NoDevice(), None, None
    return s


def test_constants():
    assert kzg.BLS_MODULUS == R and kzg.FIELD_ELEMENTS_PER_BLOB == K.N and kzg.BYTES_PER_BLOB == 131072
    assert kzg.bit_reversal_permutation(list(range(K.N))) == [K.brp(i) for i in range(K.N)]
    assert kzg.bit_reversal_permutation([7]) == [7]


def test_compute_challenge_transcript():
    blob = K.blob_bytes(K.random_blob(0xC4A1))
    commitment = bytes(range(48))
    data = b"FSBLOBVERIFY_V1_" + (4096).to_bytes(16, "big") + blob + commitment
    assert len(data) == 131152
    want = int.from_bytes(hashlib.sha256(data).digest(), "big") % R
    assert kzg.compute_challenge(blob, commitment) == want
    assert kzg.KzgSetup.compute_challenge(bytearray(blob), memoryview(commitment)) == want
    with pytest.raises(AssertionError):
        kzg.compute_challenge(blob[:-1], commitment)
    with pytest.raises(AssertionError):
        kzg.compute_challenge(blob, commitment + b"\0")


def test_blob_is_canonical():
    f = K.random_blob(0xCA70)
    assert kzg.blob_is_canonical(K.blob_bytes(f))
    assert kzg.blob_is_canonical(K.blob_bytes([R - 1] * K.N)) and kzg.blob_is_canonical(BLOB)
    for pos in (0, 2048, K.N - 1):
        for v in (R, R + 1, 1 << 255, (1 << 256) - 1, R + (1 << 64), R + (1 << 192)):
            g = list(f)
            g[pos] = v
            assert not kzg.blob_is_canonical(K.blob_bytes(g)), (pos, hex(v))


def test_lengths_and_ranges_assert_before_the_device(setup):
    z, y = bytes(32), bytes(32)
    bad_fe = R.to_bytes(32, "big")
    calls = [
        lambda: setup.blob_to_kzg_commitment(BLOB[:-1]),
        lambda: setup.blob_to_kzg_commitment(BLOB + b"\0"),
        lambda: setup.compute_kzg_proof(BLOB[:-32], z),
        lambda: setup.compute_kzg_proof(BLOB, z + b"\0"),
        lambda: setup.compute_kzg_proof(BLOB, bad_fe),
        lambda: setup.compute_kzg_proof(BLOB, b"\xff" * 32),
        lambda: setup.compute_blob_kzg_proof(BLOB, G1[:-1]),
        lambda: setup.compute_blob_kzg_proof(BLOB[1:], G1),
        lambda: setup.verify_kzg_proof(G1 + b"\0", z, y, G1),
        lambda: setup.verify_kzg_proof(G1, z, y, G1[:47]),
        lambda: setup.verify_kzg_proof(G1, z[:31], y, G1),
        lambda: setup.verify_kzg_proof(G1, z, y + b"\0", G1),
        lambda: setup.verify_kzg_proof(G1, bad_fe, y, G1),
        lambda: setup.verify_kzg_proof(G1, z, bad_fe, G1),
        lambda: setup.verify_kzg_proof_batch([G1, G1], [z], [y, y], [G1, G1]),
        lambda: setup.verify_kzg_proof_batch([G1], [z], [y], []),
        lambda: setup.verify_kzg_proof_batch([G1, G1], [z, bad_fe], [y, y], [G1, G1]),
        lambda: setup.verify_blob_kzg_proof(BLOB[:-1], G1, G1),
        lambda: setup.verify_blob_kzg_proof(BLOB, G1 + b"\0", G1),
        lambda: setup.verify_blob_kzg_proof(BLOB, G1, G1[:-1]),
        lambda: setup.verify_blob_kzg_proof_batch([BLOB], [G1, G1], [G1]),
        lambda: setup.verify_blob_kzg_proof_batch([BLOB, BLOB], [G1, G1], [G1]),
        lambda: setup.evaluate_polynomial_in_evaluation_form([0] * (K.N - 1), 5),
        lambda: setup.evaluate_polynomial_in_evaluation_form([0] * K.N, R),
        lambda: setup.evaluate_polynomial_in_evaluation_form([0] * (K.N - 1) + [R], 5),
        lambda: setup.evaluate_polynomial_in_evaluation_form(BLOB[:-1], 5),
    ]
    for n, call in enumerate(calls):
        with pytest.raises(AssertionError):
            call()
            pytest.fail("case %d reached no assertion" % n)
    # well-formed inputs do go to the device; empty lists do not
    with pytest.raises(RuntimeError, match="device call"):
        setup.verify_kzg_proof(G1, z, y, G1)
    with pytest.raises(RuntimeError, match="device call"):
        setup.blob_to_kzg_commitment(BLOB)
    assert setup.verify_kzg_proof_batch([], [], [], []) is True
    assert setup.verify_blob_kzg_proof_batch([], [], []) is True
    assert setup.blob_to_kzg_commitments([]) == [] and setup.compute_blob_kzg_proofs([], []) == []


def test_setup_argument_checks():
    with pytest.raises(ValueError):
        kzg.KzgSetup([G1] * 4095, bytes(96), ctx=NoDevice())
    with pytest.raises(AssertionError):
        kzg.KzgSetup([G1[:-1]] * 4096, bytes(96), ctx=NoDevice())
    with pytest.raises(ValueError):
        kzg.KzgSetup.verify_only(bytes(95), ctx=NoDevice())


def test_install_and_uninstall(setup):
    def own_verify(*a):
        return "own"

    spec = types.SimpleNamespace(FIELD_ELEMENTS_PER_BLOB=4096, verify_kzg_proof=own_verify,
                                 compute_challenge="own challenge", BLSFieldElement=lambda v: ("fe", v),
                                 KZGProof=lambda b: ("proof", b))
    before = dict(vars(spec))
    kzg.install(spec, setup)
    for name in kzg.PUBLIC:
        assert callable(getattr(spec, name)), name
    assert spec.verify_kzg_proof is not own_verify
    blob = K.blob_bytes(K.random_blob(0x1257))
    assert spec.compute_challenge(blob, G1) == ("fe", kzg.compute_challenge(blob, G1))  # the module's own type
    with pytest.raises(AssertionError):
        spec.verify_kzg_proof(G1, bytes(31), bytes(32), G1)
    with pytest.raises(RuntimeError, match="device call"):
        spec.compute_blob_kzg_proof(BLOB, G1)  # the installed function is the setup's
    kzg.install(spec, setup)  # a second install keeps the first one's saved originals
    kzg.uninstall(spec)
    assert dict(vars(spec)) == before
    kzg.uninstall(spec)  # nothing installed: nothing to do
    assert dict(vars(spec)) == before


def test_install_refuses_other_blob_sizes(setup):
    for spec in (types.SimpleNamespace(FIELD_ELEMENTS_PER_BLOB=4), types.SimpleNamespace()):
        before = dict(vars(spec))
        with pytest.raises(ValueError):
            kzg.install(spec, setup)
        assert dict(vars(spec)) == before
