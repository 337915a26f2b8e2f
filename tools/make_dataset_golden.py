"""Record the order in which the REFERENCE's own dataset lists a directory:

    python tools/make_dataset_golden.py        (where the reference checkout is; CPU, a second)

  tests/golden/dataset_listing.json    per listing case of tests/dataset_fixtures.py, the basenames of CustomDataset.initialize's
                                       label_paths / image_paths / orient_paths (data/custom_dataset.py:43-70,
                                       data/pix2pix_dataset.py:23-52, data/image_folder.py:16-64)

What runs: the reference's `data` package as imported (tools/make_loader_golden.py's way in), over the directory that
tests/test_data_resident.py writes again for michigan_amd.data.list_dataset.  Names only: nothing of the reference is restated here.
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "dataset_listing.json")

import dataset_fixtures as DF  # noqa: E402
from make_loader_golden import reference_data  # noqa: E402


if __name__ == "__main__":
    _, cd, _ = reference_data()
    rec = {}
    for case in DF.LISTING_CASES:
        with tempfile.TemporaryDirectory() as root:
            over = DF.write_listing_dir(root, case)
            ds = cd.CustomDataset()
            ds.initialize(DF.dataset_options(root, **over), step=1)
            rec[case] = DF.names({"label": ds.label_paths, "image": ds.image_paths, "orient": ds.orient_paths})
            print("%-18s %s" % (case, rec[case]["label"]))
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
