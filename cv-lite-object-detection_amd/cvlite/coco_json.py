"""COCO instances JSON -> the per-image ground-truth dicts the evaluation drivers read
(cvlite.evaluate "drivers"), with the standard library's json only.

  read_coco_json(path, category_ids=None) -> one dict per entry of "images", in file order:
      image_id, file_name, orig_dim [h, w]
      bbox  [N, 4] fp32  COCO's (x, y, w, h) in pixels -> (yc, xc, h, w) normalised by the image size
      label [N] int64    the index of the annotation's category_id in the sorted category ids
      iscrowd [N] uint8, area [N] fp32 (COCO's `area`: the mask area, original pixels^2)

category_ids: the categories to keep (default: every id under "categories"); an annotation of another
category is left out.  The caller adds `image` (and `img_dim`, when the resize does not fill the
padded input) after its own decode + resize; reading VOC XML is not covered.
"""
import json

import numpy as np


def read_coco_json(path, category_ids=None):
    with open(path, "r") as f:
        data = json.load(f)
    if category_ids is None:
        category_ids = [c["id"] for c in data.get("categories", [])]
    index = {cid: i for i, cid in enumerate(sorted(set(int(c) for c in category_ids)))}
    per_image = {}
    for ann in data.get("annotations", []):
        if int(ann["category_id"]) in index:
            per_image.setdefault(ann["image_id"], []).append(ann)
    out = []
    for im in data["images"]:
        h, w = float(im["height"]), float(im["width"])
        anns = per_image.get(im["id"], [])
        box = np.array([a["bbox"] for a in anns], np.float64).reshape(-1, 4)         # x, y, w, h
        bbox = np.stack([(box[:, 1] + box[:, 3] / 2.0) / h, (box[:, 0] + box[:, 2] / 2.0) / w, box[:, 3] / h,
                         box[:, 2] / w], 1).astype(np.float32)
        out.append(dict(image_id=im["id"], file_name=im["file_name"], orig_dim=[int(im["height"]), int(im["width"])],
                        bbox=bbox, label=np.array([index[int(a["category_id"])] for a in anns], np.int64),
                        iscrowd=np.array([int(a.get("iscrowd", 0)) for a in anns], np.uint8),
                        area=np.array([a.get("area", a["bbox"][2] * a["bbox"][3]) for a in anns], np.float32)))
    return out
