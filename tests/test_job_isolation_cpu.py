"""The inputs of the job-isolation tests (job_isolation_inputs.py) against the CPU oracle: every pending batch
rejects exactly the item its builder says, in every form, and every interleaved call's expected value is what the
oracle computes for the same arguments.  No GPU: test_gpu_job_isolation.py then compares the device with these."""
import pytest

import job_isolation_inputs as J
from oracle import bls_oracle_c as OC


@pytest.mark.parametrize("variant", ["bad3", "good", "bad6"])
@pytest.mark.parametrize("form", J.FORMS)
def test_pending_batches_reject_exactly_the_item_they_name(form, variant):
    p = J.pending(form, variant)
    got = [int(OC.FastAggregateVerify(*p.item(j))) for j in range(J.B)]
    want = [1] * J.B
    if J.BAD[variant] is not None:
        want[J.BAD[variant]] = 0
    assert got == p.expect == want
    assert len(p.sigs) == 96 * J.B and p.offs[-1] == p.idx.size == sum(len(m) for m in p.members)


def test_pending_batches_have_the_shapes_the_forms_need():
    for form in J.FORMS:
        p = J.pending(form, "bad3")
        assert all(0 <= k < J.N_REG for m in p.members for k in m) and all(m for m in p.members)
        assert J.pending(form, "good").sigs != p.sigs and J.pending(form, "good").members == p.members
        assert J.replacing(form).item_msgs != p.item_msgs  # a batch of its own, not the pending one again
    sh = J.pending("shared", "bad3")
    assert len(sh.table) == J.M_SHARED < J.B and sorted(set(sh.msg_ids)) == list(range(J.M_SHARED))
    bits = J.pending("bits", "bad3")
    lists = J.committee_lists()
    assert len(lists) == J.N_COMM and sorted(k for c in lists for k in c) == list(range(J.N_REG))
    for ids, bf, mem in zip(bits.committee_ids, bits.bits, bits.members):
        pool = [k for c in ids for k in lists[c]]
        assert bf.size == len(pool) and mem == [k for k, on in zip(pool, bf) if on]
    # complement mode is chosen when fewer members are absent than present: items 0 and 1
    assert int(bits.bits[0].sum()) == 8 and int(bits.bits[1].sum()) == 7 and int(bits.bits[2].sum()) == 1
    assert len(bits.committee_ids[5]) == 2
    keys = J.pending("keys", "bad3")
    assert len({k for m in keys.members for k in m}) < J.B * J.N_KEYS  # the table deduplicates


@pytest.mark.parametrize("name", list(J.CALLS))
def test_interleaved_calls_expect_what_the_oracle_computes(name):
    call = J.CALLS[name]
    assert call.want() == call.oracle()


def test_the_call_table_covers_every_route_the_job_shares():
    assert len(J.CALLS) == 22 and set(J.REPLACING) == set(J.FORMS)
    failing = [n for n in J.CALLS if n.endswith("_failing")]
    assert sorted(failing) == ["pairing_check_failing", "verify_cells_failing", "verify_failing",
                               "verify_kzg_proof_batch_failing"]
