"""Child process of tests/test_gpu_bf16_step_contract.py: the cases named on the command line, one step each under whatever
switches the environment sets (they are read once per process), through the same staged walk.  Prints one line
`STEP {case: {"worst": {stage kind: [largest |error| / bound, buffer]}, "forms": ..., "wgrad_fork": ...}}`."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from test_gpu_bf16_step_contract import run_case  # noqa: E402

if __name__ == "__main__":
    out = {}
    for name in sys.argv[1:]:
        r = run_case(name, repeats=False)
        out[name] = {"worst": {k: [v[0], str(v[1])] for k, v in r["worst"].items()}, "forms": r["forms"], "wgrad_fork": r["wgrad_fork"]}
    print("STEP " + json.dumps(out))
