"""``load_obj_tsv`` with the reference's name, signature and return value (src/utils.py:17-62): the HOST reader of the
bottom-up feature files (``train2014_obj36.tsv``, ``vg_gqa_obj36.tsv`` ...).  One line per image, ten tab-separated fields,
six of them base64 text.  It is the oracle of the device reader (``tools.tsv.load_obj_tsv_device``) and what a line the
kernel flags is redone with; written with ``bytes.split``, ``base64.b64decode`` and ``np.frombuffer`` instead of the
reference's ``csv.DictReader``."""
import base64
import time

import numpy as np

FIELDNAMES = ["img_id", "img_h", "img_w", "objects_id", "objects_conf",
              "attrs_id", "attrs_conf", "num_boxes", "boxes", "features"]

# the six base64 fields in the file's order: (name, trailing shape per box, dtype); src/utils.py:41-48
DECODE_CONFIG = (("objects_id", (), np.int64), ("objects_conf", (), np.float32), ("attrs_id", (), np.int64),
                 ("attrs_conf", (), np.float32), ("boxes", (4,), np.float32), ("features", (-1,), np.float32))


def decode_item(fields):
    """ten ``bytes`` fields of one line -> the reference's item dict (read-only arrays); raises what ``b64decode``,
    ``np.frombuffer`` and ``reshape`` raise on a malformed field (``binascii.Error`` is a ``ValueError``)"""
    item = dict(zip(FIELDNAMES, fields))
    item["img_id"] = item["img_id"].decode("utf-8")
    for key in ("img_h", "img_w", "num_boxes"):
        item[key] = int(item[key])
    boxes = item["num_boxes"]
    for key, shape, dtype in DECODE_CONFIG:
        arr = np.frombuffer(base64.b64decode(item[key]), dtype=dtype).reshape((boxes,) + shape)
        arr.setflags(write=False)
        item[key] = arr
    return item


def load_obj_tsv(fname, topk=None):
    """Load object features from a tsv file -> a list of dicts under ``FIELDNAMES`` (``topk``: only the first K lines; None
    or -1: all).  Blank lines are skipped; a line without ten fields raises ValueError naming the file and the line."""
    data = []
    start_time = time.time()
    print("Start to load Faster-RCNN detected objects from %s" % fname)
    with open(fname, "rb") as f:
        for i, line in enumerate(f):
            line = line.rstrip(b"\r\n")
            if not line:
                continue
            fields = line.split(b"\t")
            if len(fields) != len(FIELDNAMES):
                raise ValueError("%s, line %d: %d tab-separated fields, %d expected" % (fname, i + 1, len(fields), len(FIELDNAMES)))
            data.append(decode_item(fields))
            if topk is not None and len(data) == topk:
                break
    print("Loaded %d images in file %s in %d seconds." % (len(data), fname, time.time() - start_time))
    return data
