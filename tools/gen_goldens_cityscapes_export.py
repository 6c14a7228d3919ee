#!/usr/bin/env python3
"""Golden: the two tables the reference's `save_preds` maps a train-id prediction through, as its `datasets/cityscapes_config.py`
defines them, written to tests/golden/cityscapes_export_tables.json:
  train_id_to_id     [20] label id per train id, the last entry (the ignore class) 0;
  train_id_to_color  [20][3] RGB per train id, the last entry black.
tests/test_seg_export.py checks segmentation.TRAIN_ID_TO_ID / TRAIN_ID_TO_COLOR (derived from the public label definition)
against it.

    python tools/gen_goldens_cityscapes_export.py <reference checkout>

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
    ids = [int(v) for v in mod.train_id_to_id]
    colors = [[int(c) for c in row] for row in mod.train_id_to_color]
    out = os.path.join(ROOT, "tests", "golden", "cityscapes_export_tables.json")
    with open(out, "w") as f:
        f.write('{\n "source": "datasets/cityscapes_config.py: train_id_to_id, train_id_to_color",\n')
        f.write(' "train_id_to_id": ' + json.dumps(ids) + ',\n')
        f.write(' "train_id_to_color": ' + json.dumps(colors) + '\n}\n')
    print("wrote", out, len(ids), "ids,", len(colors), "colours")


if __name__ == "__main__":
    main(sys.argv)
