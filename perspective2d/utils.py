"""Import-compatible alias of the two drawing helpers the reference's demo and notebooks call right after `inference`
(`from perspective2d.utils import draw_perspective_fields, draw_from_r_p_f_cx_cy`, demo/demo.py), on the MI355X implementation: thin wrappers
that upload, call perspectivefields_amd.draw_perspective_fields / draw_camera and download.  They take numpy pictures and return numpy pictures;
code that keeps its pictures on the device calls the native functions and saves both copies.

The drawing is this library's own model (include/pf_hip.h pf_draw_fields), not matplotlib's: the same three things are
shown -- latitude colours, iso-latitude lines, up arrows -- but not pixel for pixel.  Only the arguments that the record kept in this repository
settles are taken: the positional ones, `color` / `up_color`, `density`, `arrow_inv_len` and `mode`.  Whatever further keywords the reference's
functions have (colours of the latitude layer, opacities, ...) are left out here and not guessed; the native functions have their own."""
import numpy as np
import torch

from perspectivefields_amd.engine import PfError
from perspectivefields_amd.perspectivefields import draw_camera as _draw_camera
from perspectivefields_amd.perspectivefields import draw_perspective_fields as _draw
from perspectivefields_amd.perspectivefields import general_vfov_to_focal


def _picture(img_rgb):
    img = np.ascontiguousarray(img_rgb)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"img_rgb must be a uint8 (H, W, 3) array; got {img.dtype} {img.shape}")
    if not torch.cuda.is_available():
        raise PfError("perspective2d.utils draws on the GPU only (no CPU path)")
    return torch.from_numpy(img).cuda()


def _colour(c):
    return {} if c is None else {"arrow_color": tuple(255.0 * float(v) for v in c)}


def draw_perspective_fields(img_rgb, up, latimap, color=None, density=10, arrow_inv_len=20):
    """img_rgb: numpy uint8 (H, W, 3); up: (2, H, W), the layout of `pred_gravity_original`, a tensor on any device or an array; latimap: the
    latitude (H, W) in RADIANS, as the demo passes it (`torch.deg2rad(pred["pred_latitude_original"])`; the native function takes degrees);
    color: the arrows' RGB in 0 - 1 floats, default green.  Returns a numpy uint8 (H, W, 3) picture.
    The latitude goes back to degrees in float64 and is rounded to float32 once, so it differs from the degrees the caller started from by the
    float32 roundings of its own deg2rad: at most 1.2e-5 degrees at 90."""
    img = _picture(img_rgb)
    up = torch.as_tensor(up).to(device=img.device, dtype=torch.float32)
    lat = torch.rad2deg(torch.as_tensor(latimap).to(device=img.device, dtype=torch.float64)).to(torch.float32)
    return _draw(img, up, lat, density=density, arrow_inv_len=arrow_inv_len, **_colour(color)).cpu().numpy()


def draw_from_r_p_f_cx_cy(img_rgb, roll, pitch, vfov, rel_cx, rel_cy, mode="deg", up_color=None):
    """The fields of the camera (roll, pitch, general vertical field of view, relative principal point) drawn over img_rgb (numpy uint8
    (H, W, 3)); angles in degrees unless mode="rad".  The focal length comes from `general_vfov_to_focal`, as in the reference
    (utils/utils.py:325-381).  up_color: the arrows' RGB in 0 - 1 floats, default green.  Returns a numpy uint8 (H, W, 3) picture."""
    if mode not in ("deg", "rad"):
        raise ValueError("mode must be 'deg' or 'rad'")
    img = _picture(img_rgb)
    focal = float(general_vfov_to_focal(rel_cx, rel_cy, np.degrees(vfov) if mode == "rad" else vfov))
    return _draw_camera(img, roll, pitch, focal, rel_cx, rel_cy, mode=mode, **_colour(up_color)).cpu().numpy()
