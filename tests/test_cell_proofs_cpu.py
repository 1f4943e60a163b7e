"""Host side of the cell proof functions of bls_mi355x.kzg_cells with no device: the constructor's argument errors,
the spec's assertions that are decided before any device call (the stub context raises a RuntimeError on the first
one), empty batches, install_cell_proofs / uninstall_cell_proofs on a module-like object, and the new symbols in the
shim's library list."""
import types

import pytest

import kzg_inputs as K
from bls_mi355x import _native, batch, kzg_cells

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
    s = kzg_cells.CellProofSetup.__new__(kzg_cells.CellProofSetup)
    s.ctx, s.table, s.first = NoDevice(), None, None
    return s


def test_constants_and_names():
    assert kzg_cells.PUBLIC == ("verify_cell_kzg_proof_batch", "compute_cells", "recover_cells")
    assert kzg_cells.PUBLIC_PROOFS == ("compute_cells_and_kzg_proofs", "recover_cells_and_kzg_proofs")
    assert 1 <= kzg_cells.PROOF_BLOBS_PER_MSM <= 8 and 63 * kzg_cells.PROOF_BLOBS_PER_MSM <= 511
    for name in kzg_cells.PUBLIC_PROOFS:
        assert callable(getattr(kzg_cells.CellProofSetup, name))
        assert callable(getattr(kzg_cells.CellProofSetup, name + "_batch"))
    assert callable(batch.g1_fft) and callable(kzg_cells.g1_monomial_from_lagrange)


def test_the_library_list_has_the_new_symbols():
    for name in ("bls_g1_fft", "bls_kzg_cell_proofs_setup", "bls_kzg_compute_cells_and_proofs",
                 "bls_kzg_recover_cells_and_proofs"):
        assert name in _native._SIGS, name
    assert len(_native._SIGS["bls_g1_fft"][1]) == 6
    assert len(_native._SIGS["bls_kzg_cell_proofs_setup"][1]) == 3
    assert len(_native._SIGS["bls_kzg_compute_cells_and_proofs"][1]) == 6
    assert len(_native._SIGS["bls_kzg_recover_cells_and_proofs"][1]) == 8


def test_constructor_argument_errors():
    pts = [G1] * 4096
    with pytest.raises(ValueError, match="exactly one"):
        kzg_cells.CellProofSetup(NoDevice())
    with pytest.raises(ValueError, match="exactly one"):
        kzg_cells.CellProofSetup(NoDevice(), g1_monomial=pts, g1_lagrange=pts)
    for bad in (pts[:-1], pts + [G1], []):
        with pytest.raises(ValueError, match="4,096"):
            kzg_cells.CellProofSetup(NoDevice(), g1_monomial=bad)
        with pytest.raises(ValueError, match="4,096"):
            kzg_cells.CellProofSetup(NoDevice(), g1_lagrange=bad)
    with pytest.raises(AssertionError):
        kzg_cells.CellProofSetup(NoDevice(), g1_monomial=pts[:-1] + [G1[:-1]])
    # well-formed arguments reach the device: the table for the monomial form, the transform for the Lagrange form
    with pytest.raises(RuntimeError, match="device call"):
        kzg_cells.CellProofSetup(NoDevice(), g1_monomial=pts)
    with pytest.raises(RuntimeError, match="device call"):
        kzg_cells.CellProofSetup(NoDevice(), g1_lagrange=pts)


def test_monomial_derivation_argument_errors():
    with pytest.raises(ValueError, match="4,096"):
        kzg_cells.g1_monomial_from_lagrange([G1] * 4095, NoDevice())
    with pytest.raises(AssertionError):
        kzg_cells.g1_monomial_from_lagrange([G1] * 4095 + [G1 + b"\0"], NoDevice())
    with pytest.raises(RuntimeError, match="device call"):
        kzg_cells.g1_monomial_from_lagrange([G1] * 4096, NoDevice())


def test_g1_fft_argument_errors():
    with pytest.raises(ValueError):
        batch.g1_fft([G1, G1[:-1]], ctx=NoDevice())
    with pytest.raises(ValueError):
        batch.g1_fft([[G1, G1], [G1]], ctx=NoDevice())
    with pytest.raises(RuntimeError, match="device call"):
        batch.g1_fft([G1, G1], ctx=NoDevice())


def test_computation_asserts_before_the_device(setup):
    for blob in (BLOB[:-1], BLOB + b"\0", BLOB[:-32] + BAD_FE, BAD_FE + BLOB[32:]):
        with pytest.raises(AssertionError):
            setup.compute_cells_and_kzg_proofs(blob)
        with pytest.raises(AssertionError):
            setup.compute_cells_and_kzg_proofs_batch([BLOB, blob])
    with pytest.raises(RuntimeError, match="device call"):
        setup.compute_cells_and_kzg_proofs(BLOB)
    assert setup.compute_cells_and_kzg_proofs_batch([]) == []


def test_recovery_asserts_before_the_device(setup):
    half = list(range(64))
    calls = [
        lambda: setup.recover_cells_and_kzg_proofs(half[:63], [CELL] * 63),                     # fewer than half
        lambda: setup.recover_cells_and_kzg_proofs(half, [CELL] * 63),                          # unequal lengths
        lambda: setup.recover_cells_and_kzg_proofs(half[:63], [CELL] * 64),
        lambda: setup.recover_cells_and_kzg_proofs(list(range(129)), [CELL] * 129),             # more than 128
        lambda: setup.recover_cells_and_kzg_proofs(half[:63] + [62], [CELL] * 64),              # a duplicate
        lambda: setup.recover_cells_and_kzg_proofs([1, 0] + half[2:], [CELL] * 64),             # not ascending
        lambda: setup.recover_cells_and_kzg_proofs(half[:63] + [128], [CELL] * 64),             # out of range
        lambda: setup.recover_cells_and_kzg_proofs(half, [CELL] * 63 + [CELL[:-1]]),            # a cell's length
        lambda: setup.recover_cells_and_kzg_proofs(half, [CELL] * 63 + [CELL[:-32] + BAD_FE]),  # not canonical
        lambda: setup.recover_cells_and_kzg_proofs_batch(half, [[CELL] * 64, [CELL] * 65]),     # another count
    ]
    for n, call in enumerate(calls):
        with pytest.raises(AssertionError):
            call()
            pytest.fail("case %d reached no assertion" % n)
    with pytest.raises(RuntimeError, match="device call"):
        setup.recover_cells_and_kzg_proofs(half, [CELL] * 64)
    with pytest.raises(RuntimeError, match="device call"):
        setup.recover_cells_and_kzg_proofs(list(range(128)), [CELL] * 128)
    assert setup.recover_cells_and_kzg_proofs_batch(half, []) == []


def spec_like(**kw):
    return types.SimpleNamespace(FIELD_ELEMENTS_PER_CELL=64, CELLS_PER_EXT_BLOB=128, **kw)


def test_install_and_uninstall(setup):
    spec = spec_like(compute_cells_and_kzg_proofs="own compute", recover_cells_and_kzg_proofs="own recover",
                     compute_cells="left alone", verify_cell_kzg_proof_batch="left alone too")
    before = dict(vars(spec))
    kzg_cells.install_cell_proofs(spec, setup)
    for name in kzg_cells.PUBLIC_PROOFS:
        assert callable(getattr(spec, name)), name
    assert spec.compute_cells == "left alone" and spec.verify_cell_kzg_proof_batch == "left alone too"
    with pytest.raises(AssertionError):
        spec.compute_cells_and_kzg_proofs(BLOB[:-1])
    with pytest.raises(RuntimeError, match="device call"):
        spec.compute_cells_and_kzg_proofs(BLOB)  # the installed function is the setup's
    with pytest.raises(RuntimeError, match="device call"):
        spec.recover_cells_and_kzg_proofs(list(range(64)), [CELL] * 64)
    kzg_cells.install_cell_proofs(spec, setup)  # a second install keeps the first one's saved originals
    kzg_cells.uninstall_cell_proofs(spec)
    assert dict(vars(spec)) == before
    kzg_cells.uninstall_cell_proofs(spec)  # nothing installed: nothing to do
    assert dict(vars(spec)) == before


def test_names_are_replaced_only_where_present(setup):
    spec = spec_like(recover_cells_and_kzg_proofs="own")
    before = dict(vars(spec))
    kzg_cells.install_cell_proofs(spec, setup)
    assert not hasattr(spec, "compute_cells_and_kzg_proofs") and callable(spec.recover_cells_and_kzg_proofs)
    kzg_cells.uninstall_cell_proofs(spec)
    assert dict(vars(spec)) == before
    bare = spec_like()
    kzg_cells.install_cell_proofs(bare, setup)
    assert not any(hasattr(bare, name) for name in kzg_cells.PUBLIC_PROOFS)
    kzg_cells.uninstall_cell_proofs(bare)
    assert dict(vars(bare)) == dict(vars(spec_like()))


def test_install_uses_the_modules_types(setup, monkeypatch):
    spec = spec_like(Cell=lambda b: ("cell", len(b)), KZGProof=lambda b: ("proof", len(b)),
                     compute_cells_and_kzg_proofs=None, recover_cells_and_kzg_proofs=None)
    monkeypatch.setattr(setup, "compute_cells_and_kzg_proofs", lambda blob: ([CELL, CELL], [G1, G1]))
    monkeypatch.setattr(setup, "recover_cells_and_kzg_proofs", lambda idx, cells: ([CELL], [G1]))
    kzg_cells.install_cell_proofs(spec, setup)
    assert spec.compute_cells_and_kzg_proofs(BLOB) == ([("cell", 2048)] * 2, [("proof", 48)] * 2)
    assert spec.recover_cells_and_kzg_proofs([], []) == ([("cell", 2048)], [("proof", 48)])
    kzg_cells.uninstall_cell_proofs(spec)
    assert spec.compute_cells_and_kzg_proofs is None and spec.recover_cells_and_kzg_proofs is None


def test_both_installs_on_one_module_are_independent(setup):
    cells = kzg_cells.CellSetup.__new__(kzg_cells.CellSetup)
    cells.ctx, cells.table, cells.first = NoDevice(), None, None
    spec = spec_like(compute_cells="a", recover_cells="b", verify_cell_kzg_proof_batch="c",
                     compute_cells_and_kzg_proofs="d", recover_cells_and_kzg_proofs="e")
    before = dict(vars(spec))
    kzg_cells.install_cells(spec, cells)
    assert spec.compute_cells_and_kzg_proofs == "d"  # install_cells leaves the proof forms alone
    kzg_cells.install_cell_proofs(spec, setup)
    kzg_cells.uninstall_cells(spec)
    assert spec.compute_cells == "a" and callable(spec.compute_cells_and_kzg_proofs)
    kzg_cells.uninstall_cell_proofs(spec)
    assert dict(vars(spec)) == before


def test_install_refuses_other_sizes(setup):
    for spec in (types.SimpleNamespace(FIELD_ELEMENTS_PER_CELL=64, CELLS_PER_EXT_BLOB=64),
                 types.SimpleNamespace(FIELD_ELEMENTS_PER_CELL=32, CELLS_PER_EXT_BLOB=128),
                 types.SimpleNamespace(CELLS_PER_EXT_BLOB=128), types.SimpleNamespace()):
        before = dict(vars(spec))
        with pytest.raises(ValueError):
            kzg_cells.install_cell_proofs(spec, setup)
        assert dict(vars(spec)) == before
