"""MI355X-native (gfx950) PerspectiveFields dense-field + ParamNet inference path.

    from perspectivefields_amd import PerspectiveFields      # or: from perspective2d import PerspectiveFields
    m = PerspectiveFields("Paramnet-360Cities-edina-centered").eval().cuda()
    pred = m.inference(img_bgr)
    upright = m.level_panorama(pano)                          # rotate_panorama / panorama_fields / gravity_from_views: panorama -> panorama

Sub-modules: config (zoo / cfg), schema (checkpoint keys), synth (seeded checkpoints and images),
engine (ctypes binding of libpf_hip.so), ops (kernel-level entry points), dist (image-level data
parallelism), build (hipcc build of csrc/), perspectivefields (the model class), and the geometry that
needs no model: fields (fields from camera parameters), camera_fit, field_metrics, placement (scores,
search, compositing), draw, gathers (crops, rotations, re-projections, cube maps, fisheye frames,
panorama composition, the transport of fields between cameras and onto panoramas, on one host skeleton), yaw (yaw alignment, gravity from views).
"""
__all__ = ["PerspectiveFields", "model_zoo", "fields_from_params", "fit_camera_params", "fit_camera_shared", "crop_panorama", "reproject_image", "compose_panorama", "rotate_panorama", "panorama_fields", "gravity_from_views", "crop_cubemap", "cubemap_to_panorama", "panorama_to_cubemap", "cubemap_face_cameras", "cubemap_to_image", "cubemap_from_image", "fisheye_lens", "dual_fisheye_lenses", "crop_fisheye", "fisheye_to_panorama", "yaw_scores", "align_yaw", "yaw_tree", "placement_scores", "placement_search", "transform_fields", "composite_objects", "draw_perspective_fields", "draw_camera", "field_errors", "FieldErrorAccumulator"]


# public name -> the module that defines it.  panorama_to_fisheye, fisheye_fields, fit_fisheye_lens, fisheye_lens_from_fit, reproject_fields and
# compose_panorama_fields are public through this table alone: __all__ keeps its 32 names
_HOME = {
    "PerspectiveFields": "perspectivefields", "model_zoo": "config",
    "fields_from_params": "fields",
    "fit_camera_params": "camera_fit", "fit_camera_shared": "camera_fit", "fit_fisheye_lens": "camera_fit", "fisheye_lens_from_fit": "camera_fit",
    "field_errors": "field_metrics", "FieldErrorAccumulator": "field_metrics",
    "placement_scores": "placement", "placement_search": "placement", "transform_fields": "placement", "composite_objects": "placement",
    "draw_perspective_fields": "draw", "draw_camera": "draw",
    "crop_panorama": "gathers", "reproject_image": "gathers", "compose_panorama": "gathers", "rotate_panorama": "gathers", "panorama_fields": "gathers",
    "crop_cubemap": "gathers", "cubemap_to_panorama": "gathers", "panorama_to_cubemap": "gathers", "cubemap_face_cameras": "gathers",
    "cubemap_to_image": "gathers", "cubemap_from_image": "gathers",
    "fisheye_lens": "gathers", "dual_fisheye_lenses": "gathers", "crop_fisheye": "gathers", "fisheye_to_panorama": "gathers",
    "panorama_to_fisheye": "gathers", "fisheye_fields": "gathers", "reproject_fields": "gathers", "compose_panorama_fields": "gathers",
    "yaw_scores": "yaw", "align_yaw": "yaw", "yaw_tree": "yaw", "gravity_from_views": "yaw",
}


def __getattr__(name):  # lazy: keeps `import perspectivefields_amd.synth` free of torch
    if name not in _HOME:
        raise AttributeError(name)
    from importlib import import_module
    obj = globals()[name] = getattr(import_module("." + _HOME[name], __name__), name)   # kept: the next access does not come here
    return obj
