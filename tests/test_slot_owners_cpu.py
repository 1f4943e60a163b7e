"""Static guard of the scratch slots a submitted FAV batch still needs until its finish.

Job 0 is shared: every per-call entry point, the curve, aggregation, table, signing-root and KZG calls run on its
streams and claim scratch slots there (SCR(S_x, n, ptr) in csrc/*.hip), and a batch submitted through the job API
may sit on the same job between its submit and its finish.  KEPT_SLOTS lists, from reading fav_finish, fav_bisect,
read_own, job_partial and enqueue_comm_check (csrc/bls_capi.hip, csrc/bls_capi_comm.hip), the slots those read
after the submit has returned.  A claim of one of them anywhere but in the functions that own the batch's state
would let another call rewrite (or, by growing the slot, free) what the finish reads: this test finds such a claim
by the slot's name.  test_gpu_job_isolation.py checks the same rule by running the calls."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eth-consensus-specs_amd", "csrc")

# slot -> what reads it after the submit
KEPT_SLOTS = {
    "S_STATUS": "fav_finish writes the verdicts of a passing batch from it; fav_bisect gates every leaf on it",
    "S_RSC": "fav_bisect copies the r_i to rebuild -r_i G1 for the signature side of every leaf",
    "S_RP": "fav_bisect reads r_i apk_i back for the per-item Miller values (shared-message and shared-f batches)",
    "S_H": "fav_bisect reads H(m) back, per item or through S_MSGID per message",
    "S_SIG": "fav_bisect copies the decoded signatures for e(-r_i G1, sigma_i)",
    "S_FAV_F": "fav_bisect takes the batch's own per-item f as the leaves' hash side (one pair per f)",
    "S_MSGID": "fav_bisect gathers a shared-message batch's per-item H through the items' message ids",
    "S_BYTES": "bls_fav_job_check_comm all-gathers the partial's bytes when the job was submitted before the "
               "communicator existed",
    "S_OWN": "the own check's verdict word: enqueue_own_check copies it to the host behind the check",
    "S_OWN_F": "read_own checks this copy of the job's product when the submit left the own check for later "
               "(device exchange); S_FPART itself is claimed by every per-call product",
    "S_BITEM": "bls_last_gather_work reads a bits batch's item records back",
}

# function -> why its claims of kept slots are the batch's own
ALLOWED = {
    "fav_scratch": "sizes every slot of the batch that fav_prepare is about to enqueue: the submit itself",
    "fav_bisect": "the finish's own reader",
    "job_submit": "the submit: the partial's bytes and the copy of the product the own check reads",
    "enqueue_own_check": "claims the own check's verdict word, from job_submit or read_own",
    "enqueue_comm_check": "the submit's device exchange",
}
# (function, slot) exceptions, each with its reason
ALLOWED_PAIRS = {
    ("bls_committees_load", "S_BITEM"): "resets bits_B first, so bls_last_gather_work reads no batch's records "
                                        "there, and waits for the device before it touches the table",
}
# bls_capi_test.hip: the test hooks say in include/blsmi355x.h that they use the FAV batch's scratch and may not run
# between a batch's partial and finish calls
ALLOWED_FILES = {"bls_capi_test.hip"}

CLAIM = re.compile(r"\bSCR\(\s*(S_[A-Z0-9_]+)\s*,")
FUNC = re.compile(r"^(?!//|#|\}|extern\b|namespace\b|using\b|template\b|struct\b|enum\b|static_assert\b)"
                  r"[A-Za-z_][^;]*?\b([A-Za-z_][\w:]*)\s*\(")


def slot_enum():
    text = open(os.path.join(CSRC, "bls_capi_internal.h")).read()
    body = re.search(r"enum Slot \{(.*?)\n\};", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    return [s.strip() for s in body.split(",") if s.strip()]


def claims():
    """(file, line number, enclosing function, slot) of every SCR(S_x, ...) in csrc/*.hip"""
    out = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        func = None
        for no, line in enumerate(open(path), 1):
            if line[:1] not in (" ", "\t", "\n"):
                m = FUNC.match(line)
                if m and not line.rstrip().endswith(";"):
                    func = m.group(1).split("::")[-1]
            for slot in CLAIM.findall(line):
                out.append((os.path.basename(path), no, func, slot))
    return out


def test_every_kept_slot_exists():
    names = slot_enum()
    assert names[-1] == "NSLOT" and len(names) == len(set(names))
    assert [s for s in KEPT_SLOTS if s not in names] == []
    assert all(KEPT_SLOTS.values()) and all(ALLOWED.values()) and all(ALLOWED_PAIRS.values())


def test_the_scan_sees_the_claims_it_is_about():
    found = claims()
    assert len(found) > 300  # every C ABI piece claims its scratch this way
    by_func = {}
    for _, _, func, slot in found:
        by_func.setdefault(func, set()).add(slot)
    # the owners, by name: if one is renamed the allow list must follow
    assert {"S_STATUS", "S_RSC", "S_RP", "S_H", "S_SIG", "S_FAV_F", "S_MSGID", "S_BITEM"} <= by_func["fav_scratch"]
    assert {"S_BYTES", "S_OWN_F"} <= by_func["job_submit"]
    assert by_func["enqueue_own_check"] == {"S_OWN"}
    assert "S_BITEM" in by_func["bls_committees_load"]
    assert "S_PC_P" in by_func["verify_percall"] and "S_AV_F" in by_func["bls_aggregate_verify_batch"]
    assert all(func for _, _, func, _ in found)
    # every claimed name is a slot
    assert {slot for *_, slot in found} <= set(slot_enum())


def test_kept_slots_are_claimed_only_by_the_batch_itself():
    bad = [(f, no, func, slot) for f, no, func, slot in claims()
           if slot in KEPT_SLOTS and f not in ALLOWED_FILES and func not in ALLOWED
           and (func, slot) not in ALLOWED_PAIRS]
    assert bad == [], "a call outside the FAV batch's own functions claims a slot a pending batch still reads"


def test_the_own_check_reads_its_own_copy_of_the_product():
    """read_own may run long after the submit: it must not read S_FPART, which every per-call product claims"""
    text = open(os.path.join(CSRC, "bls_capi.hip")).read()
    body = text[text.index("static int read_own("):text.index("static int job_partial(")]
    assert "S_OWN_F" in body and "S_FPART" not in body
