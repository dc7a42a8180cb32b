"""Subprocess body of test_gpu_nf_cells.py::test_nf_group_form_against_the_gather_form: GGML_MI355X_NF_GROUPS is read once per process, so the parent sets it to 0 before
this process loads the backend.  Runs every probe of nf_ref.GROUP_CASES, gates each one, writes the results to the .npz named on the command line and prints one JSON line."""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import llama_box_amd as L  # noqa: E402
import nf_ref as NR  # noqa: E402


def main():
    H = L.host()
    be = L.Backend(0)
    res, bad = {}, []
    for cid in NR.GROUP_CASES:
        case = next(c for c in NR.CASES if c.id == cid)
        probes = NR.indicator_probes(case) + NR.witness_probes(case) + NR.witness_probes(case, True) + [NR.random_probe(case)]
        for p in probes:
            got, wrong = NR.run_counted(case, p, be, H)
            if wrong:
                bad.append(wrong)
            if p.name != "random":
                try:
                    NR.check_probe(case, p, got)
                except AssertionError as e:
                    bad.append(str(e))
            res[f"{cid}|{p.name}"] = got
    np.savez(sys.argv[1], **res)
    be.close()
    print("NF_GROUPS_JSON " + json.dumps({"env": os.environ.get("GGML_MI355X_NF_GROUPS"), "probes": len(res), "bad": bad[:12]}))


if __name__ == "__main__":
    main()
