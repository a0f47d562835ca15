"""tests/golden/train_args.json: the argparse defaults of the REAL reference train.py (its
main(), train.py:178-217), read by stopping its own parser after parse_args([]). Settings only.
Needs a checkout of the reference:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_args.py <reference checkout>
(or AACLIP_REFERENCE=<reference checkout>)."""
import argparse
import importlib.util
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ["AACLIP_REFERENCE"])
sys.path.insert(0, os.path.join(HERE, "stubs"))
sys.path.insert(0, REFERENCE)
sys.dont_write_bytecode = True


class _Parsed(Exception):
    pass


def main():
    if importlib.util.find_spec("tqdm") is None:  # only its name is needed to import train.py
        sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda it, *a, **k: it)
    prev = os.getcwd()
    os.chdir(REFERENCE)
    try:
        spec = importlib.util.spec_from_file_location("reference_train", os.path.join(REFERENCE, "train.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        os.chdir(prev)
    real = argparse.ArgumentParser.parse_args

    def capture(self, args=None, namespace=None):
        raise _Parsed(vars(real(self, [], namespace)))

    argparse.ArgumentParser.parse_args = capture
    try:
        mod.main()
    except _Parsed as e:
        defaults = e.args[0]
    finally:
        argparse.ArgumentParser.parse_args = real
    out = {"generated_by": "tests/golden/make_golden_train_args.py (reference train.py main(), parse_args([]))",
           "defaults": defaults}
    with open(os.path.join(HERE, "train_args.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(defaults, sort_keys=True))


if __name__ == "__main__":
    main()
