"""Perspective fields from camera parameters on the GPU (pf_fields_from_params), and the closed form from the general vertical FoV to the focal length."""
from __future__ import annotations

import numpy as np
import torch

from .engine import PfError


def fields_from_params(roll, pitch, rel_focal, rel_cx=0.0, rel_cy=0.0, height=None, width=None, mode="deg", device=None, xi=0.0):
    """Camera parameters -> (up field (2,H,W) unit vectors, latitude map (H,W) in degrees) on the GPU: the step the
    reference's demos run right after inference (utils/utils.py:325-381 -> PanoCam.get_up_general / get_lat_general,
    utils/panocam.py:451-556), e.g. to compare the ParamNet output with the predicted fields.  Same layout and units as
    `pred_gravity_original` / `pred_latitude_original`.  Arguments may be Python floats or 0-d tensors (the `pred_*`
    entries of an inference dict: they stay on the device, no host round trip); angles in degrees unless mode="rad".

    xi: mirror parameter of the Unified Spherical Model (the `xi` of crop_panorama, `pred_xi` of fit_camera_params(distortion=True)).
    The Python number 0 (the default) is the pinhole model above.  Anything else -- a non-zero number or a tensor, which stays on the
    device and is not looked at on the host -- synthesises the USM fields of include/pf_hip.h pf_fields_from_params_usm: NaN where a
    pixel has no ray (xi > 1), and for a tensor that holds 0 the same bits as the pinhole call."""
    from .engine import _check, _stream_ptr, load_library

    if height is None or width is None:
        raise ValueError("fields_from_params needs the output size (height, width)")
    dev = None
    usm = torch.is_tensor(xi) or float(xi) != 0.0
    for v in (roll, pitch, rel_focal, rel_cx, rel_cy, xi):
        if torch.is_tensor(v) and v.is_cuda:
            dev = v.device
    if dev is None:
        dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise PfError("fields_from_params runs on the GPU only (no CPU path)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    t = [torch.as_tensor(v, dtype=torch.float64).to(dev).reshape(()) for v in (roll, pitch, rel_focal, rel_cx, rel_cy) + ((xi,) if usm else ())]
    if mode == "deg":
        t[0], t[1] = torch.deg2rad(t[0]), torch.deg2rad(t[1])
    elif mode != "rad":
        raise ValueError("mode must be 'deg' or 'rad'")
    cam = torch.stack(t).to(torch.float32).contiguous()
    up = torch.empty((2, int(height), int(width)), dtype=torch.float32, device=dev)
    lat = torch.empty((int(height), int(width)), dtype=torch.float32, device=dev)
    lib = load_library()
    entry = "pf_fields_from_params_usm" if usm else "pf_fields_from_params"
    with torch.cuda.device(dev):
        _check(getattr(lib, entry)(dev.index, cam.data_ptr(), int(height), int(width), up.data_ptr(), lat.data_ptr(), _stream_ptr()), None, entry)
    return up, lat


def general_vfov_to_focal(rel_cx, rel_cy, gvfov_deg):
    """Relative focal length from the general vertical FoV (reference: utils/utils.py:47-91 with h=1,
    degree=True).  With u = f^2 + cx^2 + cy^2 + 1/4 the reference's equation
    cos(gvfov) = (u - 1/2) / sqrt(u^2 - cy^2) is a quadratic in u, solved here in closed form
    (the reference runs scipy.fsolve from 1.5 on the same equation and returns |f|)."""
    cx = np.asarray(rel_cx, dtype=np.float64)
    cy = np.asarray(rel_cy, dtype=np.float64)
    c = np.cos(np.radians(np.asarray(gvfov_deg, dtype=np.float64)))
    s2 = 1.0 - c * c
    disc = np.sqrt(np.maximum(1.0 - 4.0 * s2 * (c * c * cy * cy + 0.25), 0.0))
    # root selection: cos > 0 needs u > 1/2 -> '+' root; cos < 0 (gvfov > 90 deg) -> '-' root
    u = np.where(c >= 0, (1.0 + disc), (1.0 - disc)) / (2.0 * s2)
    f2 = u - cy * cy - 0.25 - cx * cx
    return np.sqrt(np.abs(f2))
