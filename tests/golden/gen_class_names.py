"""Generate tests/golden/class_names.json: the label lists the reference's test.py / demo.py draw with.

    python tests/golden/gen_class_names.py [path/to/reference]     (default: $YN_REFERENCE, else ../reference beside the repository)

"voc" is data/voc.py's VOC_CLASSES; "coco" is coco_class_labels[coco_class_index[i]] for the 80 class indices i the network
predicts (data/coco.py; the indirection of test.py:79-81 resolved).  Names only: tests/test_draw_cpu.py checks that the built-in font
covers every character of them.  The product never reads the file.  data/voc.py and data/coco.py import cv2 for their image loading,
which this generator never calls, so a missing cv2 is replaced by an empty stub module for the import.
"""
import importlib.util
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("YN_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
OUT = os.path.join(ROOT, "tests", "golden", "class_names.json")


def load(name):
    spec = importlib.util.spec_from_file_location("yn_ref_data_" + name, os.path.join(REF, "data", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    try:
        import cv2  # noqa: F401
    except ImportError:
        sys.modules["cv2"] = types.ModuleType("cv2")
    voc, coco = load("voc"), load("coco")
    names = {"voc": list(voc.VOC_CLASSES), "coco": [coco.coco_class_labels[i] for i in coco.coco_class_index]}
    assert len(names["voc"]) == 20 and len(names["coco"]) == 80
    with open(OUT, "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
