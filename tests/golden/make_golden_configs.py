"""Generate tests/golden/reference_configs.json: the reference's own configs/car_cfg.py and configs/multi_cfg.py as
sassd.config.Config.fromfile loads them (unmodified files), and the parameter list of the detector build_detector makes
from each -- the data tests/test_reference_configs_cpu.py compares this repo's configs/ against.

    python tests/golden/make_golden_configs.py <reference checkout>

Tuples are stored as {"__tuple__": [...]} so that the loaded structure round-trips exactly.  Dataset / work-dir path
keys (PATH_KEYS) are dropped and every other path string keeps only its file name behind "<dir>/": they name
directories on the reference authors' machines, and the test ignores both.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import sassd  # noqa: E402,F401
from sassd.config import Config  # noqa: E402
from sassd.detector import build_detector  # noqa: E402

NAMES = ("car_cfg.py", "multi_cfg.py")
PATH_KEYS = {"root", "ann_file", "img_prefix", "data_root", "db_info_path", "work_dir", "filename", "load_from",
             "resume_from", "save_to_file"}


def encode(v):
    if isinstance(v, dict):
        return {k: encode(x) for k, x in v.items() if k not in PATH_KEYS}
    if isinstance(v, tuple):
        return {"__tuple__": [encode(x) for x in v]}
    if isinstance(v, list):
        return [encode(x) for x in v]
    if isinstance(v, str) and "/" in v:
        return "<dir>/" + os.path.basename(v)
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


def main(ref_root):
    out = {}
    for name in NAMES:
        cfg = Config.fromfile(os.path.join(ref_root, "configs", name))
        model = build_detector(cfg.model, cfg.train_cfg, cfg.test_cfg)
        out[name] = {"config": encode(cfg),
                     "state_dict": [[k, list(t.shape)] for k, t in model.state_dict().items()],
                     "num_parameters": sum(p.numel() for p in model.parameters())}
    with open(os.path.join(HERE, "reference_configs.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print({k: (len(v["state_dict"]), v["num_parameters"]) for k, v in out.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
