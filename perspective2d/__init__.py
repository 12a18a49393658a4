"""Import-compatible alias so that the reference's documented entry point
(`from perspective2d import PerspectiveFields`, reference perspective2d/__init__.py:1,
README.md:98-112) resolves to the MI355X implementation."""
from perspectivefields_amd.perspectivefields import PerspectiveFields, align_yaw, compose_panorama, composite_objects, crop_fisheye, draw_camera, draw_perspective_fields, dual_fisheye_lenses, fisheye_fields, fisheye_lens, fisheye_lens_from_fit, fisheye_to_panorama, fit_fisheye_lens, model_zoo, panorama_to_fisheye, placement_scores, placement_search, rotate_panorama, transform_fields  # noqa: F401
