"""Child process of tests/test_gpu_f32_step_contract.py: the cases named on the command line, one step each under whatever
switches the environment sets (they are read once per process), through the same staged walk.  With HIG_TEXT_FORK=0 the forward
goes through hig_denoiser_fwd_text, the one entry that switch changes.  Prints one line
`STEP {case: {"worst": {stage kind: [largest |error| / bound, buffer]}, "sched_f": ..., "sched_b": ..., "sha": {result: sha256}}}`."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from test_gpu_f32_step_contract import run_case  # noqa: E402

if __name__ == "__main__":
    out = {}
    for name in sys.argv[1:]:
        r = run_case(name, repeats=False, one_call=os.environ.get("HIG_TEXT_FORK") == "0")
        out[name] = {"worst": {k: [v[0], str(v[1])] for k, v in r["worst"].items()}, "sched_f": r["sched_f"], "sched_b": r["sched_b"], "sha": r["sha"]}
    print("STEP " + json.dumps(out))
