#!/usr/bin/env python3
"""Golden for the drop-in tests (tests/test_dropin.py), recorded from the reference checkout (build container only).

    python tests/golden/make_dropin_golden.py REFERENCE_CHECKOUT   ->  tests/golden/reference_cli.json

Stores data only:
  option_defaults   vars(option.args) of the reference's option.py when it is imported with no arguments (it parses at import time)
  eval_sh_argv      the argument list eval.sh passes to main.py, split as a shell would split it
  checkout_modules  the top-level module names the reference's checkout provides next to main.py (*.py files and directories)
  model_files       the module files of the checkout's own model/ directory, which the shim has to shadow
"""
import json
import os
import shlex
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tests/golden/make_dropin_golden.py REFERENCE_CHECKOUT")
    ref = os.path.abspath(sys.argv[1])
    code = "import sys, json; sys.argv=['x']; import option; print(json.dumps(vars(option.args)))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ref, capture_output=True, text=True, check=True)
    defaults = json.loads(r.stdout)
    eval_sh = open(os.path.join(ref, "eval.sh")).read()
    argv = shlex.split(eval_sh.split("main.py", 1)[1].replace("\\\n", " "))
    modules = sorted(n[:-3] if n.endswith(".py") else n for n in os.listdir(ref)
                     if (n.endswith(".py") or os.path.isdir(os.path.join(ref, n))) and not n.startswith((".", "_")))
    model_files = sorted(n for n in os.listdir(os.path.join(ref, "model")) if n.endswith(".py"))
    out = os.path.join(HERE, "reference_cli.json")
    with open(out, "w") as f:
        json.dump({"option_defaults": defaults, "eval_sh_argv": argv, "checkout_modules": modules, "model_files": model_files}, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
