"""Generate tests/golden/stereoscene_config.json from the REFERENCE's own config file
(projects/configs/occupancy/semantickitti/stereoscene.py with its two _base_ files), evaluated the way mmcv's Config does:
each file executed, bases merged in order, the file's own keys merged over them.  The values only (data, no source): the
CPU tests build the pipelines, the runner arguments and the model from it without the reference checkout.  Tuples are
stored as {"__tuple__": [...]} so that they come back as tuples.
Run:  PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden_config.py"""
import json
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import REF  # noqa: E402

CFG = "projects/configs/occupancy/semantickitti/stereoscene.py"
OUT = os.path.join(ROOT, "tests", "golden", "stereoscene_config.json")


def _merge(base, child):
    out = dict(base)
    for k, v in child.items():
        if isinstance(v, dict) and isinstance(out.get(k), dict) and not v.get("_delete_", False):
            out[k] = _merge(out[k], v)
        else:
            out[k] = {x: y for x, y in v.items() if x != "_delete_"} if isinstance(v, dict) else v
    return out


def load(path):
    ns = runpy.run_path(path)
    own = {k: v for k, v in ns.items() if not k.startswith("__") and not callable(v) and not isinstance(v, type(os))}
    bases = own.pop("_base_", [])
    merged = {}
    for b in [bases] if isinstance(bases, str) else bases:
        merged = _merge(merged, load(os.path.normpath(os.path.join(os.path.dirname(path), b))))     # every base must exist
    return _merge(merged, own)


def encode(v):
    if isinstance(v, dict):
        return {str(k): encode(x) for k, x in v.items()}
    if isinstance(v, tuple):
        return {"__tuple__": [encode(x) for x in v]}
    if isinstance(v, list):
        return [encode(x) for x in v]
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


def main():
    cfg = load(os.path.join(REF, CFG))
    from stereoscene_amd.registry import Config
    assert Config._load(os.path.join(REF, CFG)) == cfg, "the product's loader disagrees with the mmcv-style evaluation"
    with open(OUT, "w") as f:
        json.dump({"_doc": f"values of the reference's {CFG} with its _base_ files merged (oracle/make_golden_config.py)",
                   "source": CFG, "config": encode(cfg)}, f, indent=1, sort_keys=False)
        f.write("\n")
    print("wrote", os.path.relpath(OUT, ROOT), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
