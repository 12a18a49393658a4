"""MI355X-native (gfx950) PerspectiveFields dense-field + ParamNet inference path.

    from perspectivefields_amd import PerspectiveFields      # or: from perspective2d import PerspectiveFields
    m = PerspectiveFields("Paramnet-360Cities-edina-centered").eval().cuda()
    pred = m.inference(img_bgr)
    upright = m.level_panorama(pano)                          # rotate_panorama / panorama_fields / gravity_from_views: panorama -> panorama

Sub-modules: config (zoo / cfg), schema (checkpoint keys), synth (seeded checkpoints and images),
engine (ctypes binding of libpf_hip.so), ops (kernel-level entry points), dist (image-level data
parallelism), build (hipcc build of csrc/).
"""
__all__ = ["PerspectiveFields", "model_zoo", "fields_from_params", "fit_camera_params", "fit_camera_shared", "crop_panorama", "reproject_image", "compose_panorama", "rotate_panorama", "panorama_fields", "gravity_from_views", "crop_cubemap", "cubemap_to_panorama", "panorama_to_cubemap", "cubemap_face_cameras", "cubemap_to_image", "cubemap_from_image", "fisheye_lens", "dual_fisheye_lenses", "crop_fisheye", "fisheye_to_panorama", "yaw_scores", "align_yaw", "yaw_tree", "placement_scores", "placement_search", "transform_fields", "composite_objects", "draw_perspective_fields", "draw_camera", "field_errors", "FieldErrorAccumulator"]


def __getattr__(name):  # lazy: keeps `import perspectivefields_amd.synth` free of torch
    if name == "PerspectiveFields":
        from .perspectivefields import PerspectiveFields

        return PerspectiveFields
    if name == "fields_from_params":
        from .perspectivefields import fields_from_params

        return fields_from_params
    if name == "fit_camera_params":
        from .perspectivefields import fit_camera_params

        return fit_camera_params
    if name == "fit_camera_shared":
        from .perspectivefields import fit_camera_shared

        return fit_camera_shared
    if name == "crop_panorama":
        from .perspectivefields import crop_panorama

        return crop_panorama
    if name == "reproject_image":
        from .perspectivefields import reproject_image

        return reproject_image
    if name == "compose_panorama":
        from .perspectivefields import compose_panorama

        return compose_panorama
    if name in ("rotate_panorama", "panorama_fields", "gravity_from_views"):
        from . import perspectivefields as _pfm

        return getattr(_pfm, name)
    if name in ("crop_cubemap", "cubemap_to_panorama", "panorama_to_cubemap", "cubemap_face_cameras", "cubemap_to_image", "cubemap_from_image"):
        from . import perspectivefields as _pfm

        return getattr(_pfm, name)
    if name in ("fisheye_lens", "dual_fisheye_lenses", "crop_fisheye", "fisheye_to_panorama"):
        from . import perspectivefields as _pfm

        return getattr(_pfm, name)
    if name in ("yaw_scores", "align_yaw", "yaw_tree"):
        from . import perspectivefields as _pfm

        return getattr(_pfm, name)
    if name == "placement_scores":
        from .perspectivefields import placement_scores

        return placement_scores
    if name in ("placement_search", "transform_fields", "composite_objects"):
        from . import perspectivefields as _pfm

        return getattr(_pfm, name)
    if name in ("draw_perspective_fields", "draw_camera"):
        from . import perspectivefields as _pfm

        return getattr(_pfm, name)
    if name == "field_errors":
        from .perspectivefields import field_errors

        return field_errors
    if name == "FieldErrorAccumulator":
        from .perspectivefields import FieldErrorAccumulator

        return FieldErrorAccumulator
    if name == "model_zoo":
        from .config import model_zoo

        return model_zoo
    raise AttributeError(name)
