"""Host side of bls_mi355x.kzg_cells with no device: the assertions that are decided before any device call (the stub
context raises a RuntimeError on the first one), the commitments' deduplication, and install_cells /
uninstall_cells on a module-like object."""
import types

import pytest

import kzg_inputs as K
from bls_mi355x import kzg_cells

R = K.R
G1 = K.IDENTITY48
CELL = bytes(kzg_cells.BYTES_PER_CELL)
BLOB = bytes(131072)
BAD_FE = R.to_bytes(32, "big")


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
    s = kzg_cells.CellSetup.__new__(kzg_cells.CellSetup)
    s.ctx, s.table, s.first = NoDevice(), None, None
    return s


def test_constants():
    assert kzg_cells.BLS_MODULUS == R
    assert kzg_cells.BYTES_PER_CELL == 2048 and kzg_cells.BYTES_PER_EXT_BLOB == 2 * 131072
    assert kzg_cells.ITEMS_MAX >= 8192 and kzg_cells.BLOBS_MAX >= 64
    assert kzg_cells.PUBLIC == ("verify_cell_kzg_proof_batch", "compute_cells", "recover_cells")


def test_dedupe_commitments():
    a, b, c = bytes([1]) * 48, bytes([2]) * 48, bytes([3]) * 48
    assert kzg_cells.dedupe_commitments([b, a, b, c, a, a]) == ([b, a, c], [0, 1, 0, 2, 1, 1])
    assert kzg_cells.dedupe_commitments([]) == ([], [])
    assert kzg_cells.dedupe_commitments([a]) == ([a], [0])


def test_verification_asserts_before_the_device(setup):
    bad_cell = CELL[:-32] + BAD_FE
    calls = [
        lambda: setup.verify_cell_kzg_proof_batch([G1, G1], [0], [CELL, CELL], [G1, G1]),
        lambda: setup.verify_cell_kzg_proof_batch([G1], [0], [CELL], []),
        lambda: setup.verify_cell_kzg_proof_batch([G1], [0, 1], [CELL], [G1]),
        lambda: setup.verify_cell_kzg_proof_batch([G1[:-1]], [0], [CELL], [G1]),
        lambda: setup.verify_cell_kzg_proof_batch([G1], [0], [CELL], [G1 + b"\0"]),
        lambda: setup.verify_cell_kzg_proof_batch([G1], [0], [CELL[:-1]], [G1]),
        lambda: setup.verify_cell_kzg_proof_batch([G1], [0], [CELL + b"\0"], [G1]),
        lambda: setup.verify_cell_kzg_proof_batch([G1], [128], [CELL], [G1]),
        lambda: setup.verify_cell_kzg_proof_batch([G1], [-1], [CELL], [G1]),
        lambda: setup.verify_cell_kzg_proof_batch([G1], [0], [bad_cell], [G1]),
        lambda: setup.verify_cell_kzg_proof_batch([G1, G1], [0, 1], [CELL, BAD_FE + CELL[32:]], [G1, G1]),
        lambda: setup.verify_cell_kzg_proof_items([G1], [0], [b"\xff" * 2048], [G1]),
    ]
    for n, call in enumerate(calls):
        with pytest.raises(AssertionError):
            call()
            pytest.fail("case %d reached no assertion" % n)
    with pytest.raises(RuntimeError, match="device call"):
        setup.verify_cell_kzg_proof_batch([G1], [127], [CELL], [G1])
    assert setup.verify_cell_kzg_proof_batch([], [], [], []) is True
    assert setup.verify_cell_kzg_proof_items([], [], [], []) == []


def test_cell_computation_asserts_before_the_device(setup):
    for blob in (BLOB[:-1], BLOB + b"\0", BLOB[:-32] + BAD_FE, BAD_FE + BLOB[32:]):
        with pytest.raises(AssertionError):
            setup.compute_cells(blob)
        with pytest.raises(AssertionError):
            kzg_cells.compute_cells_batch([BLOB, blob], NoDevice())
    with pytest.raises(RuntimeError, match="device call"):
        setup.compute_cells(BLOB)
    assert setup.compute_cells_batch([]) == []


def test_recovery_asserts_before_the_device(setup):
    half = list(range(64))
    calls = [
        lambda: setup.recover_cells(half[:63], [CELL] * 63),                      # fewer than half
        lambda: setup.recover_cells(half, [CELL] * 63),                           # unequal lengths
        lambda: setup.recover_cells(half[:63], [CELL] * 64),
        lambda: setup.recover_cells(list(range(129)), [CELL] * 129),              # more than 128
        lambda: setup.recover_cells(half[:63] + [62], [CELL] * 64),               # a duplicate
        lambda: setup.recover_cells([1, 0] + half[2:], [CELL] * 64),              # not ascending
        lambda: setup.recover_cells(half[:63] + [128], [CELL] * 64),              # an index out of range
        lambda: setup.recover_cells(half, [CELL] * 63 + [CELL[:-1]]),             # a cell's length
        lambda: setup.recover_cells(half, [CELL] * 63 + [CELL[:-32] + BAD_FE]),   # a non-canonical element
        lambda: setup.recover_cells_batch(half, [[CELL] * 64, [CELL] * 65]),      # one blob with another count
    ]
    for n, call in enumerate(calls):
        with pytest.raises(AssertionError):
            call()
            pytest.fail("case %d reached no assertion" % n)
    with pytest.raises(RuntimeError, match="device call"):
        setup.recover_cells(half, [CELL] * 64)
    with pytest.raises(RuntimeError, match="device call"):
        setup.recover_cells(list(range(128)), [CELL] * 128)
    assert setup.recover_cells_batch(half, []) == []


def test_setup_argument_checks():
    with pytest.raises(ValueError):
        kzg_cells.CellSetup(NoDevice(), [G1] * 63, bytes(96))
    with pytest.raises(AssertionError):
        kzg_cells.CellSetup(NoDevice(), [G1[:-1]] * 64, bytes(96))
    with pytest.raises(ValueError):
        kzg_cells.CellSetup(NoDevice(), [G1] * 64, bytes(95))


def spec_like(**kw):
    return types.SimpleNamespace(FIELD_ELEMENTS_PER_CELL=64, CELLS_PER_EXT_BLOB=128, **kw)


def test_install_and_uninstall(setup):
    def own_verify(*a):
        return "own"

    spec = spec_like(verify_cell_kzg_proof_batch=own_verify, compute_cells="own cells", Cell=lambda b: ("cell", b),
                     compute_cells_and_kzg_proofs="left alone")
    before = dict(vars(spec))
    kzg_cells.install_cells(spec, setup)
    for name in kzg_cells.PUBLIC:
        assert callable(getattr(spec, name)), name
    assert spec.verify_cell_kzg_proof_batch is not own_verify
    assert spec.compute_cells_and_kzg_proofs == "left alone"
    with pytest.raises(AssertionError):
        spec.verify_cell_kzg_proof_batch([G1], [128], [CELL], [G1])
    with pytest.raises(RuntimeError, match="device call"):
        spec.compute_cells(BLOB)  # the installed function is the setup's
    with pytest.raises(RuntimeError, match="device call"):
        spec.recover_cells(list(range(64)), [CELL] * 64)
    kzg_cells.install_cells(spec, setup)  # a second install keeps the first one's saved originals
    kzg_cells.uninstall_cells(spec)
    assert dict(vars(spec)) == before
    kzg_cells.uninstall_cells(spec)  # nothing installed: nothing to do
    assert dict(vars(spec)) == before


def test_install_uses_the_modules_cell_type(setup, monkeypatch):
    spec = spec_like(Cell=lambda b: ("cell", len(b)), compute_cells=None)
    monkeypatch.setattr(setup, "compute_cells", lambda blob: [CELL, CELL])
    monkeypatch.setattr(setup, "recover_cells", lambda idx, cells: [CELL])
    kzg_cells.install_cells(spec, setup)
    assert spec.compute_cells(BLOB) == [("cell", 2048)] * 2
    assert spec.recover_cells([], []) == [("cell", 2048)]
    kzg_cells.uninstall_cells(spec)
    assert spec.compute_cells is None and not hasattr(spec, "recover_cells")


def test_compute_cells_is_installed_only_where_the_module_has_it(setup):
    spec = spec_like(recover_cells="own")
    before = dict(vars(spec))
    kzg_cells.install_cells(spec, setup)
    assert not hasattr(spec, "compute_cells")
    assert callable(spec.recover_cells) and callable(spec.verify_cell_kzg_proof_batch)
    kzg_cells.uninstall_cells(spec)
    assert dict(vars(spec)) == before


def test_install_refuses_other_sizes(setup):
    for spec in (types.SimpleNamespace(FIELD_ELEMENTS_PER_CELL=64, CELLS_PER_EXT_BLOB=64),
                 types.SimpleNamespace(FIELD_ELEMENTS_PER_CELL=32, CELLS_PER_EXT_BLOB=128),
                 types.SimpleNamespace(CELLS_PER_EXT_BLOB=128), types.SimpleNamespace()):
        before = dict(vars(spec))
        with pytest.raises(ValueError):
            kzg_cells.install_cells(spec, setup)
        assert dict(vars(spec)) == before
