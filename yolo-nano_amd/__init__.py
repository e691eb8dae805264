"""yolo-nano_amd — MI355X-native YOLO-Nano hot path (imported as ``yolo_nano_amd``).

``arch`` / ``weights`` are torch-free; ``YOLONano`` and ``fuse_conv_bn`` (the drop-in surface of
models/yolo_nano.py and utils/fuse_conv_bn.py) are imported lazily so that the pure-python parts
stay usable without torch.
"""
from . import arch, weights  # noqa: F401


def __getattr__(name):
    if name in ("YOLONano", "fuse_conv_bn", "Conv", "ShuffleNetV2", "ShuffleV2Block", "shufflenetv2", "SGD", "multi_gt_creator", "ModelEMA", "TestTimeAugmentation", "ValTransforms", "rescale_boxes", "resize_batch"):
        from . import model
        return getattr(model, name)
    if name == "rect_window":
        from . import rect                                    # host arithmetic only
        return rect.rect_window
    if name in ("SlicedInference", "slice_grid", "tile_table"):
        from . import slicing                                 # host arithmetic until SlicedInference touches a model
        return getattr(slicing, name)
    if name in ("TrainTransforms", "ColorTransforms", "AugParams", "Mosaic", "MosaicParams"):
        from . import augment                                 # numpy only: safe to import in DataLoader workers
        return getattr(augment, name)
    if name in ("VOCEval", "evaluate", "parse_rec", "gt_array", "voc_geometry"):
        from . import voc                                     # evaluate.py would be shadowed by its own evaluate()
        return getattr(voc, name)
    if name in ("COCOEval", "coco_gt_arrays", "evaluate_coco"):
        from . import coco
        return getattr(coco, name)
    if name in ("anchor_box_kmeans", "AnchorKMeans", "dataset_boxes", "as_anchor_table"):
        from . import anchors                                 # numpy only until a device object is made
        return getattr(anchors, name)
    if name in ("Visualizer", "class_colors", "default_font"):
        from . import draw                                    # numpy only until a Visualizer is made
        return getattr(draw, name)
    if name in ("weighted_boxes_fusion", "soft_nms", "Ensemble"):
        from . import fusion                                  # numpy only until a fusion runs
        return getattr(fusion, name)
    if name in ("ChipExtractor", "unchip_boxes"):
        from . import chips                                   # numpy only until a ChipExtractor is made
        return getattr(chips, name)
    if name == "Tracker":
        from . import track                                   # numpy only until a Tracker is made
        return track.Tracker
    if name in ("JPEGDecoder", "imread", "imread_batch", "JPEGEncoder", "imencode", "imwrite", "imwrite_batch"):
        from . import jpeg                                    # files -> device frames (yn_jpeg_*), and back (yn_jpeg_enc_*)
        return getattr(jpeg, name)
    if name in ("Handle", "YnError", "YnRangeError", "load_library"):
        from . import capi
        return getattr(capi, name)
    raise AttributeError(name)
