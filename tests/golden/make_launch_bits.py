#!/usr/bin/env python3
"""Write tests/golden/launch_bits.json: what the host launch path of the block and chain entry points decides, as the library that
is built in the tree (or the one HINT_AMD_LIB names) decides it on an MI355X.

Runs at development time only, on a machine with the GPU, with a library whose bits are the ones to keep:

    python tests/golden/make_launch_bits.py [output file [an earlier recording of the same library]]

"cases": per (group of call forms, kernel family) of tests/test_gpu_call_forms.py - which runs each group against the float64
oracle first - the CU count, the resolved B, a sha256 of every generated input and of every tensor the forms hand back (z, J, x,
g_x, g_c, the flat gradients' real elements, the Adam arenas of F7; loss_acc only where the launch has at most 64 workgroups), the
dynamic LDS bytes of the group's last forward and backward launch, and the tape and workspace sizes at that B.
"faults": the message of every call of tests/test_gpu_entry_faults.py that the host refuses before a launch.
Given an earlier recording, a tensor whose digest differs between the two is left out and named under "dropped" (the test then
skips that tensor alone); inputs, sizes and messages that differ stop the script.

The file was recorded at the last commit at which apply(), hint_chain_forward_noisy, hint_chain_inverse and run_backward each wrote
out the launch sequence and the chain's four backward entry points each their own checks ("build").  Re-record only for a change
that is meant to move bits or messages, never to make the tests pass.  The fixture holds data only.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import torch
    from hint_amd import _lib
    import test_gpu_call_forms as forms
    import test_gpu_entry_faults as faults
    out = sys.argv[1] if len(sys.argv) > 1 else forms.BITS_PATH
    lib = _lib.load()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    rec = dict(build=lib.hint_build_info().decode(), cases={}, dropped=[], faults=faults.record(lib))
    for group, fam in forms.CASES:
        rec["cases"][f"{group}/{fam}"] = forms.run_case(lib, group, fam, cu)
    if len(sys.argv) > 2:
        with open(sys.argv[2]) as f:
            old = json.load(f)
        assert old["build"] == rec["build"] and old["faults"] == rec["faults"] and set(old["cases"]) == set(rec["cases"])
        for name, case in rec["cases"].items():
            was = old["cases"][name]
            assert {k: v for k, v in was.items() if k != "outputs"} == {k: v for k, v in case.items() if k != "outputs"}, name
            for k in sorted(set(case["outputs"]) | set(was["outputs"])):
                if case["outputs"].get(k) != was["outputs"].get(k):
                    case["outputs"].pop(k, None)
                    rec["dropped"].append(f"{name}:{k}")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{out}: {os.path.getsize(out)} bytes, {len(rec['cases'])} cases, {len(rec['faults'])} refused calls, dropped: {rec['dropped']}")


if __name__ == "__main__":
    main()
