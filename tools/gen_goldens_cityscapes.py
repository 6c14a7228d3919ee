#!/usr/bin/env python3
"""Golden: the Cityscapes label table (name, label id, train id) as the reference's `datasets/cityscapes_config.py` defines it,
written to tests/golden/cityscapes_train_ids.json.  tests/test_seg_eval.py checks segmentation.CITYSCAPES_LABELS (written
from the public label definition) and the id -> train-id lookup against it.

    python tools/gen_goldens_cityscapes.py <reference checkout>

Only the reference's config module is imported (it needs numpy and torch)."""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    path = os.path.join(argv[1], "datasets", "cityscapes_config.py")
    spec = importlib.util.spec_from_file_location("cityscapes_config", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows = [[c.name, int(c.id), int(c.train_id)] for c in mod.classes]
    out = os.path.join(ROOT, "tests", "golden", "cityscapes_train_ids.json")
    with open(out, "w") as f:
        json.dump({"source": "datasets/cityscapes_config.py: classes (name, id, train_id)", "classes": rows}, f, indent=1)
        f.write("\n")
    print("wrote", out, len(rows), "classes")


if __name__ == "__main__":
    main(sys.argv)
