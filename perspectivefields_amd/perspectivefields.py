"""Drop-in replacement for `perspective2d.PerspectiveFields` on MI355X.

Same surface as the reference class (perspective2d/perspectivefields.py:121-272):
`PerspectiveFields(version).eval().cuda()`, `.inference(img_bgr)`,
`.inference_batch(img_bgr_list)`, `.forward(batched_inputs)`, `.versions()`, attributes
`.version`, `.param_on`, `.cfg`, `.device`, module-level `model_zoo`; both entry points
run under no_grad and never mutate their inputs; the returned dicts have the reference's
keys, key order, shapes, dtypes (fp32) and units.

What differs by design: the nn.Module tree is replaced by one HIP engine (libpf_hip.so
through include/pf_hip.h); the checkpoint is validated strictly (the reference loads with
strict=False, :185,192); there is no network, so weights come from a local file, a
state_dict, or the seeded synthetic generator.  No CPU path exists: forward() on a CPU
device raises.
"""
from __future__ import annotations

import ctypes
import math
import operator
import os
from collections import OrderedDict
from collections.abc import Mapping
from typing import Dict, List, Optional, Union

import numpy as np
import torch
from PIL import Image
from torch import nn

from . import config as _config
from .config import NET_H, NET_W, arch_of, get_cfg, model_zoo
from .engine import Engine, PfError
from .schema import checkpoint_schema, validate_state_dict
from .synth import synthetic_state_dict


class ResizeTransform:
    """HxW(xC) image -> new_h x new_w, aspect ratio not kept (reference: ResizeTransform.apply_image, perspectivefields.py:34-66): uint8 through PIL's antialiased
    BILINEAR (single-channel HxWx1 as mode "L"); any other dtype through torch's F.interpolate (no antialiasing, align_corners=False), as the reference does because
    "PIL only supports uint8".  Host-side preprocessing, as in the reference; inference()/inference_batch() can run the uint8 form on the GPU instead (device_resize)."""

    _PIL_TO_INTERPOLATE = {Image.NEAREST: "nearest", Image.BILINEAR: "bilinear", Image.BICUBIC: "bicubic"}

    def __init__(self, new_h: int, new_w: int, interp=None):
        self.new_h, self.new_w = new_h, new_w
        self.interp = Image.BILINEAR if interp is None else interp

    def apply_image(self, img: np.ndarray, interp=None) -> np.ndarray:
        assert len(img.shape) <= 4
        method = interp if interp is not None else self.interp
        if img.dtype == np.uint8:
            if len(img.shape) > 2 and img.shape[2] == 1:
                out = np.asarray(Image.fromarray(img[:, :, 0], mode="L").resize((self.new_w, self.new_h), method))
                return np.expand_dims(out, -1)
            return np.asarray(Image.fromarray(img).resize((self.new_w, self.new_h), method))
        if any(x < 0 for x in img.strides):
            img = np.ascontiguousarray(img)
        t = torch.from_numpy(img)
        shape = list(t.shape)
        shape_4d = shape[:2] + [1] * (4 - len(shape)) + shape[2:]
        t = t.view(shape_4d).permute(2, 3, 0, 1)  # hw(c) -> nchw
        mode = self._PIL_TO_INTERPOLATE[method]
        t = torch.nn.functional.interpolate(t, (self.new_h, self.new_w), mode=mode, align_corners=None if mode == "nearest" else False)
        shape[:2] = (self.new_h, self.new_w)
        return t.permute(2, 3, 0, 1).reshape(shape).numpy()  # nchw -> hw(c)


def _resolve_weights(version: str, weights) -> Dict[str, np.ndarray]:
    """weights: None | 'synthetic' | 'synthetic:<seed>' | path | state_dict | {'model': state_dict}."""
    if isinstance(weights, str) and weights.startswith("synthetic"):
        seed = int(weights.split(":", 1)[1]) if ":" in weights else 0
        return synthetic_state_dict(version, seed)
    if isinstance(weights, dict):
        sd = weights["model"] if "model" in weights and isinstance(weights["model"], dict) else weights
        return OrderedDict(sd)
    path = weights
    if path is None:
        fname = os.path.basename(model_zoo[version]["weights"])
        candidates = []
        if os.environ.get("PF_WEIGHTS_DIR"):
            candidates.append(os.path.join(os.environ["PF_WEIGHTS_DIR"], fname))
        candidates.append(os.path.join(torch.hub.get_dir(), "checkpoints", fname))
        path = next((c for c in candidates if os.path.exists(c)), None)
        if path is None:
            raise FileNotFoundError(
                f"no local checkpoint for '{version}' (looked for {candidates}); this build has no network access. "
                f"Download {model_zoo[version]['weights']} elsewhere and point PF_WEIGHTS_DIR at it, pass weights=<path|state_dict>, "
                "or weights='synthetic' for the seeded random checkpoint used by tests and benchmarks."
            )
    ckpt = torch.load(path, map_location="cpu", weights_only=True)  # a checkpoint is tensors in dicts: never unpickle arbitrary objects from a downloaded file
    return OrderedDict(ckpt["model"] if "model" in ckpt else ckpt)


def _window_limit(r) -> float:
    """upper end of the split-f16 window for one range record: 65504, except the attention operands, which carry extra powers of two inside the kernel
    (attn.hip: q x 8, k / v x 16) -- their window ends at 8188 / 4094 -- and the inputs of the Winograd convolutions (16376)"""
    name = r["name"]
    if "[winograd]" in name:   # the input transform of the Winograd convs adds four values (wino.hip) and does not clamp
        return 65504.0 / 4.0
    if name.startswith("attention") and name.endswith(" q"):
        return 8188.0
    if name.startswith("attention") and name.endswith(" kv"):
        return 4094.0
    return 65504.0


class PerspectiveFields(nn.Module):
    def __init__(self, version: str = "Paramnet-360Cities-edina-centered", weights=None, precision: str = "auto"):
        super().__init__()
        # 'fp32' is the parity mode: fp32-class contractions on the 2-way fp16 split -- full accuracy for activations in [2^-3, 65504], saturation beyond, an
        # absolute 2^-25 per element below (sb_split.h).  'fp32_bf16x6' is the exact bf16 split (no window, ~1.5x the MFMA work).  'auto' (the DEFAULT: a checkpoint
        # outside the window must not give wrong fields silently) decides between the two ONCE, on the first batch inference() / inference_batch() / forward() see:
        # a range-recording forward (pf_debug_forward_u8) and 'fp32_bf16x6' if any dense-layer input saturates or is all-tiny, 'fp32' otherwise (`self.precision`
        # then holds the decision, `self.precision_reason` why).  The decision is NOT final: in 'auto' every later forward is watched by the engine's saturation
        # counter (pf_set_saturation_counter: the producing kernels count outputs beyond their consumer's window), and a batch that moves it is re-run in
        # 'fp32_bf16x6', where the model then stays (a warning says so).  'fp32' pins the fast mode without the watch's host synchronisation.  No reduced-precision
        # mode is offered (include/pf_hip.h pf_set_precision says why).
        if precision not in ("auto", "fp32", "fp32_bf16x6"):
            raise ValueError(f"precision must be 'auto', 'fp32' or 'fp32_bf16x6', got '{precision}'")
        self._auto = precision == "auto"
        self.precision = precision
        cfg = get_cfg(version)  # KeyError on an unknown version, as the reference (:127)
        self.version = version
        self.param_on = model_zoo[version]["param"]
        self.cfg = cfg
        self.arch = arch_of(cfg)
        self.register_buffer("pixel_mean", torch.tensor(cfg.MODEL.PIXEL_MEAN).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.tensor(cfg.MODEL.PIXEL_STD).view(-1, 1, 1), False)
        self.input_format = cfg.INPUT.FORMAT
        self.aug = ResizeTransform(cfg.DATALOADER.RESIZE[0], cfg.DATALOADER.RESIZE[1])
        # True: inference()/inference_batch() upload the original uint8 image and run the (bit-identical) PIL resize
        # on the GPU instead of on a host core (1.7 ms/image/core); same bytes reach the network either way.
        self.device_resize = os.environ.get("PF_DEVICE_RESIZE", "0") == "1"
        self._engine: Optional[Engine] = None
        self._state: Dict[str, np.ndarray] = OrderedDict()
        self._init_weights(weights)

    # -------------------------------------------------------------- reference surface
    @property
    def device(self):
        return self.pixel_mean.device

    @staticmethod
    def versions():
        for key in model_zoo:
            print(f"{key}")
            print(f"   - {model_zoo[key]['description']}")

    def _init_weights(self, weights=None):
        sd = _resolve_weights(self.version, weights)
        # a checkpoint FILE is loaded like the reference does (strict=False: extra entries tolerated, with a warning);
        # state_dicts handed over in memory and the synthetic generator are held to the exact schema
        self.load_state_dict(sd, strict=not (weights is None or (isinstance(weights, str) and not weights.startswith("synthetic"))))

    def state_dict(self, *args, **kwargs):  # checkpoint-format view (host copies)
        return OrderedDict((k, torch.as_tensor(np.asarray(v))) for k, v in self._state.items())

    def load_state_dict(self, state_dict, strict: bool = True):
        sd = state_dict["model"] if "model" in state_dict and isinstance(state_dict["model"], dict) else state_dict
        host = OrderedDict()
        for k, v in sd.items():
            host[k] = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        # missing keys / wrong shapes are always fatal; keys this architecture does not have are fatal only when strict
        # (the reference loads with strict=False, :185,192: zoo files may carry extra entries) and are dropped otherwise
        extra = validate_state_dict(self.version, host, strict=strict)
        if extra:
            import warnings

            warnings.warn(f"PerspectiveFields.load_state_dict: ignoring {len(extra)} checkpoint entries this architecture does not use: {extra[:4]}")
            for k in extra:
                host.pop(k)
        self._state = host
        self._engine = None
        return self

    def _get_engine(self) -> Engine:
        dev = self.device
        if dev.type != "cuda":
            raise PfError(
                f"PerspectiveFields is on '{dev}': the MI355X engine has no CPU path. Call .cuda() / .to('cuda:N') first."
            )
        if self._engine is None or self._engine.device != dev:
            eng = Engine(self.arch["arch_id"], dev)
            eng.load_state_dict(self._state)
            eng.set_precision("fp32" if self.precision == "auto" else self.precision)  # always: the model's precision wins over any default of the library
            self._engine = eng
        return self._engine

    @torch.no_grad()
    def inference(self, img_bgr: np.ndarray) -> dict:
        return self.inference_batch([img_bgr])[0]

    @torch.no_grad()
    def inference_batch(self, img_bgr_list: List[np.ndarray]) -> List[dict]:
        """uint8 HxWx3 images (as cv2.imread returns) take the PIL path -- bit-identical bytes on the host or on the GPU; any other dtype (float images, 0..255) follows
        the reference's other branch (perspectivefields.py:48-66): F.interpolate on the host, then the float entry point of the engine (pf_forward_f32)."""
        batch, sizes = self._prepare_batch(img_bgr_list)
        return self._run(batch, sizes)

    @torch.no_grad()
    def inference_batch_with_params(self, img_bgr_list: List[np.ndarray]):
        """inference_batch plus the engine's raw (B, 8) camera-parameter tensor (include/pf_hip.h pf_forward_u8: d_params; None without a ParamNet) -- the per-image
        rows the multi-GPU path all-gathers (dist.ShardedPerspectiveFields).  An empty list gives ([], an empty (0, 8) tensor or None)."""
        if len(img_bgr_list) == 0:
            return [], (torch.zeros((0, 8), dtype=torch.float32, device=self.device) if self.param_on else None)
        batch, sizes = self._prepare_batch(img_bgr_list)
        lazy: list = []
        results = self._run(batch, sizes, lazy_params=lazy)   # joined forwards: the parameters are complete in stream order
        params = None
        if lazy:
            for res, pr in lazy:
                for r, extra in zip(res, self._param_dicts(pr)):
                    r.update(extra)
            params = lazy[0][1] if len(lazy) == 1 else torch.cat([pr for _, pr in lazy])
        return results, params

    def _prepare_batch(self, img_bgr_list: List[np.ndarray]):
        """host images -> (network input on the device, [(H, W)]): uint8 (B,320,320,3) through PIL (or the bit-identical device resize), float (B,3,320,320) otherwise.
        A list of CUDA uint8 (H, W, 3) tensors on the model's device is resized on the device by the same bit-exact kernel whatever device_resize says."""
        if any(torch.is_tensor(im) for im in img_bgr_list):
            return self._prepare_device_batch(img_bgr_list)
        if any(im.dtype != np.uint8 for im in img_bgr_list):
            sizes, chw = [], []
            for img_bgr in img_bgr_list:
                original = img_bgr[:, :, ::-1] if self.input_format == "RGB" else img_bgr
                sizes.append(tuple(int(v) for v in original.shape[:2]))
                r = self.aug.apply_image(np.ascontiguousarray(original))
                chw.append(torch.as_tensor(np.ascontiguousarray(r.astype("float32").transpose(2, 0, 1))))   # as the reference: image.astype("float32").transpose(2, 0, 1)
            return torch.stack(chw).to(self.device), sizes
        sizes, resized = [], []
        for img_bgr in img_bgr_list:
            original = img_bgr  # never mutated: apply_image returns a new array (reference copies, :196,211)
            if self.input_format == "RGB":
                original = original[:, :, ::-1]
            sizes.append(tuple(int(v) for v in original.shape[:2]))
            resized.append(np.ascontiguousarray(original) if self.device_resize else self.aug.apply_image(np.ascontiguousarray(original)))
        if self.device_resize:
            # one upload of all original images, then the whole batch resized in two launches per 32 images
            eng = self._get_engine()
            flat = torch.from_numpy(np.concatenate([im.reshape(-1) for im in resized])).to(self.device)
            views, o = [], 0
            for im in resized:
                views.append(flat[o:o + im.size].view(im.shape))
                o += im.size
            batch = torch.empty((len(resized), NET_H, NET_W, 3), dtype=torch.uint8, device=self.device)
            eng.resize_batch_into(views, batch)
        else:
            batch = torch.from_numpy(np.stack(resized)).to(self.device, non_blocking=False)  # uint8 (B,320,320,3)
        return batch, sizes

    def _prepare_device_batch(self, imgs):
        if not all(torch.is_tensor(im) for im in imgs):
            raise TypeError("inference_batch: a list mixes numpy arrays and tensors")
        for im in imgs:
            if im.dtype != torch.uint8:
                raise TypeError(f"inference_batch takes uint8 device tensors only (got {im.dtype}); float images go through numpy")
            if im.device != self.device:
                raise ValueError(f"inference_batch: a tensor is on '{im.device}', the model on '{self.device}'")
            if im.dim() != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
                raise ValueError(f"inference_batch: images must be (H, W, 3); got {tuple(im.shape)}")
        eng = self._get_engine()
        views = [(im.flip(-1) if self.input_format == "RGB" else im).contiguous() for im in imgs]   # the numpy path's channel flip
        sizes = [(int(im.shape[0]), int(im.shape[1])) for im in imgs]
        batch = torch.empty((len(views), NET_H, NET_W, 3), dtype=torch.uint8, device=self.device)
        eng.resize_batch_into(views, batch)
        return batch, sizes

    # ------------------------------------------------------------------ debug forward (sanitizer / shadow-compare mode)
    @torch.no_grad()
    def debug_forward(self, img_bgr_list: List[np.ndarray], shadow: bool = True, ranges: bool = True):
        """The forward of `inference_batch` with the engine's debug sink (pf_debug_forward_u8): returns (results, taps, ranges).
        taps: {name: NHWC fp32 device tensor} of every block / stage boundary -- compare with `oracle.pf_oracle.forward(..., taps={})` to find the FIRST layer that
        is off; ranges: per dense layer input max |x|, rms, saturated / non-finite counts -- the first thing to run on a real checkpoint (see `check_range`)."""
        sizes = [tuple(int(v) for v in im.shape[:2]) for im in img_bgr_list]
        resized = [self.aug.apply_image(np.ascontiguousarray(im[:, :, ::-1] if self.input_format == "RGB" else im)) for im in img_bgr_list]
        batch = torch.from_numpy(np.stack(resized)).to(self.device)
        eng = self._get_engine()
        pg, pl, params, taps, rng = eng.forward_debug(batch, shadow=shadow, ranges=ranges)
        return self._assemble(eng, pg, pl, params, sizes), taps, rng

    def check_range(self, img_bgr_list: List[np.ndarray], verbose: bool = True) -> dict:
        """Range report of a checkpoint on real images.  The default precision ("fp32": 2-way fp16 split) represents |x| in [2^-3, 65504] with 22+ bits, SATURATES
        beyond 65504 and keeps only an absolute 2^-25 per element below 2^-3: a layer input with saturated elements, or whose rms is below 2^-5 (an all-tiny tensor), is
        outside the window -- use precision="fp32_bf16x6" (exact bf16 split, no window) for such a checkpoint.  Returns {"ok", "saturated", "tiny", "non_finite", "layers"}."""
        _, _, rng = self.debug_forward(img_bgr_list, shadow=False, ranges=True)
        sat = [r for r in rng if r["saturated"] > 0 or r["max_abs"] > _window_limit(r)]
        bad = [r for r in rng if r["non_finite"] > 0]
        tiny = [r for r in rng if 0.0 < r["rms"] < 2.0 ** -5]
        if verbose:
            print(f"{len(rng)} dense-layer inputs: max |x| {max((r['max_abs'] for r in rng), default=0.0):.4g}, smallest rms {min((r['rms'] for r in rng), default=0.0):.4g}; "
                  f"{len(sat)} with saturated elements, {len(tiny)} with rms < 2^-5, {len(bad)} with non-finite elements")
            for r in (sat + tiny + bad)[:20]:
                print(f"  {r['name']}: max |x| {r['max_abs']:.4g} rms {r['rms']:.4g} saturated {r['saturated']} non-finite {r['non_finite']}")
        return {"ok": not (sat or bad or tiny), "saturated": sat, "tiny": tiny, "non_finite": bad, "layers": rng}

    # ------------------------------------------------------------------ streaming
    _HOST_KEYS = ("pred_gravity", "pred_gravity_original", "pred_latitude", "pred_latitude_original")

    @torch.no_grad()
    def inference_stream(self, batches, to_host: bool = True, depth: int = 2, with_params: bool = False):
        """Pipelined inference over an iterable of image lists (see _inference_stream); leaves the engine's deferred-ParamNet mode off however the iteration ends.
        with_params: yield (results, raw (B, 8) camera-parameter tensor or None) pairs -- what dist.ShardedPerspectiveFields all-gathers."""
        try:
            yield from self._inference_stream(batches, to_host, depth, with_params)
        finally:
            eng = self._engine
            if eng is not None and getattr(eng, "defer_params", False):
                eng.set_defer_params(False)

    def _inference_stream(self, batches, to_host: bool = True, depth: int = 2, with_params: bool = False):
        """Pipelined inference over an iterable of image lists: yields one `inference_batch`-style result list per input
        batch, in order.  Three HIP streams overlap the stages of consecutive batches -- upload (pinned staging buffer,
        async H2D), compute (forward + post-process), download -- because the reference's callers move the fields to the
        host right after inference (demo/demo.py:55-58, 4.9 MB per 640x640 image).  With `to_host` the four field tensors
        of every result are pinned CPU tensors (filled by async D2H; complete when the batch is yielded); the ParamNet
        scalars stay 0-d device tensors as in `inference_batch`.  `depth` = batches in flight.
        With depth >= 2 the ParamNet branch of a batch runs on the engine's own stream beside the next batch's backbone (Engine.set_defer_params); a batch is yielded
        once ITS fields and ITS branch are complete (an event behind the branch, Engine.params_ready_event), with the scalar entries built after that."""
        dev = self.device
        if dev.type != "cuda":
            raise PfError(f"PerspectiveFields is on '{dev}': the MI355X engine has no CPU path. Call .cuda() first.")
        eng = self._get_engine()
        s_up, s_comp, s_down = (torch.cuda.Stream(device=dev) for _ in range(3))
        inflight = []
        # pinned upload staging: a ring of depth + 1 reusable buffers (a slot is rewritten only after its copy has completed)
        nslots = max(1, depth) + 1
        slots = [{"buf": None, "done": None} for _ in range(nslots)]
        nbatch = 0

        defer = self.param_on and depth >= 2
        if defer:
            eng.set_defer_params(True)
        keep_params = self.param_on and (defer or with_params)    # the scalar entries are built when a batch is finished, from its raw parameter tensors
        s_join = torch.cuda.Stream(device=dev) if keep_params else None  # waits for the deferred branches only (Engine.params_ready_event) / for the batch's own compute

        state = {"rerun_before": 0}   # batches with seq < this were issued in the fast mode before a window exit was seen: re-run unconditionally

        def finish(item):
            # With the deferred branch the camera parameters of `item` are written on the engine's own stream.  Wait for THAT branch only (an event recorded behind it on
            # s_join right after the forward was issued) -- not for the compute of the batch submitted after it, which would leave the GPU idle while the host prepares
            # the next batch -- and only then build the scalar entries: for ParamNetConvNextRegress they are arithmetic on `params` (factors), which must not be launched
            # before the branch has written them.
            if defer:
                item["params_done"].synchronize()
            item["done"].synchronize()
            rerun = False
            if item["sat"] is not None and item["fast"]:
                # precision='auto': did this batch leave the split-f16 window?  Two looks at the counter, both behind finished work (reading them costs nothing):
                # the snapshots behind each chunk's forward on the compute stream, and -- deferred branch -- one behind the BRANCH on s_join: the ParamNet kernels of batch
                # i run after snapshot i was taken (beside batch i + 1's backbone), so without it their increments would be charged to batch i + 1, or to nobody for the
                # last batch.  The counter is global: an increment seen here may belong to a later batch that is already running -- so once it moves, EVERY batch that
                # was issued in the fast mode (at most `depth` of them) is re-run in the exact mode when its turn comes, not only this one.
                snaps = [snap for snap, _, _, _ in item["sat"]] + ([item["sat_branch"]] if item["sat_branch"] is not None else [])
                moved = [self._left_window(eng, snap) for snap in snaps]
                if any(moved):
                    state["rerun_before"] = max(state["rerun_before"], nbatch)
                rerun = item["seq"] < state["rerun_before"]

            def out(res, lazy):
                if not with_params:
                    return res
                prs = [pr for _, pr in (lazy or [])]
                return res, (None if not prs else prs[0] if len(prs) == 1 else torch.cat(prs))

            if rerun:
                lz = [] if keep_params else None
                with torch.cuda.stream(s_comp):
                    new = self._rerun_exact(eng, item["batch"], item["sizes"], lz)   # joined forwards: the parameters are complete in stream order
                    for res, params in (lz or []):
                        for r, extra in zip(res, self._param_dicts(params)):
                            r.update(extra)
                    if with_params and lz:
                        lz = [(None, torch.cat([pr for _, pr in lz]))]
                s_comp.synchronize()
                for r, n in zip(item["results"], new):
                    r.clear()
                    r.update({k: (v.cpu() if (to_host and k in self._HOST_KEYS) else v) for k, v in n.items()})
                return out(item["results"], lz)
            if keep_params:
                with torch.cuda.stream(s_join):  # NOT the compute stream: it already holds the next batch's forward
                    if not defer:
                        s_join.wait_event(item["comp_done"])
                    for res, params in item["lazy"]:
                        for r, extra in zip(res, self._param_dicts(params)):
                            r.update(extra)
                    if with_params and len(item["lazy"]) > 1:
                        item["lazy"] = [(None, torch.cat([pr for _, pr in item["lazy"]]))]
                s_join.synchronize()
            return out(item["results"], item["lazy"])

        for imgs in batches:
            sizes, resized = [], []
            for img_bgr in imgs:
                original = img_bgr[:, :, ::-1] if self.input_format == "RGB" else img_bgr
                if original.dtype != np.uint8:
                    raise TypeError("PerspectiveFields expects uint8 BGR images (as cv2.imread returns)")
                sizes.append(tuple(int(v) for v in original.shape[:2]))
                resized.append(np.ascontiguousarray(original) if self.device_resize else self.aug.apply_image(np.ascontiguousarray(original)))
            slot = slots[nbatch % nslots]
            nbatch += 1
            if slot["done"] is not None:
                slot["done"].synchronize()
            nbytes = sum(int(im.size) for im in resized)
            if slot["buf"] is None or slot["buf"].numel() < nbytes:
                slot["buf"] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            host = slot["buf"]
            host_np = host.numpy()  # shares the pinned memory
            offs, o = [], 0
            for im in resized:
                np.copyto(host_np[o:o + im.size], im.reshape(-1))
                offs.append(o)
                o += int(im.size)
            with torch.cuda.stream(s_up):
                dev_in = host[:nbytes].to(dev, non_blocking=True)  # one H2D per batch
                if self.device_resize:
                    batch = torch.empty((len(resized), NET_H, NET_W, 3), dtype=torch.uint8, device=dev)
                    eng.resize_batch_into([dev_in[offs[i]:offs[i] + im.size].view(im.shape) for i, im in enumerate(resized)], batch)
                else:
                    batch = dev_in.view(len(resized), NET_H, NET_W, 3)
                up_done = torch.cuda.Event()
                up_done.record(s_up)
            slot["done"] = up_done
            batch.record_stream(s_comp)
            s_comp.wait_event(up_done)
            lazy = [] if keep_params else None
            sat = [] if self._auto else None
            with torch.cuda.stream(s_comp):
                results = self._run(batch, sizes, lazy_params=lazy, sat_out=sat)
                comp_done = torch.cuda.Event()
                comp_done.record(s_comp)
            params_done = eng.params_ready_event(s_join) if defer else None
            sat_branch = None
            if defer and sat is not None and sat:   # the counter as of the END of this batch's ParamNet branch (s_join is behind it)
                with torch.cuda.stream(s_join):
                    sat_branch = eng.saturation_snapshot()
            done = comp_done
            if to_host:
                s_down.wait_event(comp_done)
                total = sum(r[k].numel() for r in results for k in self._HOST_KEYS)
                pinned = torch.empty(total, dtype=torch.float32, pin_memory=True)  # one pinned block per batch, sliced into views
                with torch.cuda.stream(s_down):
                    o = 0
                    for r in results:
                        for k in self._HOST_KEYS:
                            src = r[k]
                            src.record_stream(s_down)
                            dst = pinned[o:o + src.numel()].view(src.shape)
                            dst.copy_(src, non_blocking=True)
                            r[k] = dst
                            o += src.numel()
                    done = torch.cuda.Event()
                    done.record(s_down)
            inflight.append({"results": results, "done": done, "comp_done": comp_done, "params_done": params_done, "lazy": lazy, "sat": sat, "sat_branch": sat_branch,
                             "batch": batch, "sizes": sizes, "seq": nbatch - 1, "fast": self.precision == "fp32"})
            if len(inflight) >= max(1, depth):
                yield finish(inflight.pop(0))
        while inflight:
            yield finish(inflight.pop(0))
        if defer:
            with torch.cuda.stream(s_comp):
                eng.set_defer_params(False)

    def fields_from_prediction(self, pred: dict, height: int, width: int):
        """Perspective fields implied by the ParamNet scalars of one inference() result (see fields_from_params)."""
        if not self.param_on:
            raise PfError(f"'{self.version}' has no ParamNet: there are no camera parameters to synthesise fields from")
        return fields_from_params(pred["pred_roll"], pred["pred_pitch"], pred["pred_rel_focal"], pred["pred_rel_cx"], pred["pred_rel_cy"],
                                  height, width, mode="deg")

    def fit_camera(self, preds, **kw):
        """Camera parameters fitted to the dense fields of one inference() result (a dict) or of an inference_batch() list, on the
        GPU (see fit_camera_params for the options and the returned entries).  Works on every zoo version, PersNet included.
        init="paramnet" starts from the result's own ParamNet scalars (ParamNet models only; at xi = 0 with distortion=True).
        shared_intrinsics=True fits the results as the frames of one camera, a list of labels (one per result) as several cameras: one
        joint fit per camera with its focal length (principal point, xi) shared, see fit_camera_shared.  Returns new dicts; the inference
        results are not changed."""
        single = isinstance(preds, dict)
        plist = [preds] if single else list(preds)
        if isinstance(kw.get("init"), str):
            if kw["init"] != "paramnet":
                raise ValueError("init must be None, 'paramnet' or a list of parameter dicts")
            if not self.param_on:
                raise PfError(f"'{self.version}' has no ParamNet: init='paramnet' needs pred_* scalars")
            kw["init"] = plist
        shared = kw.pop("shared_intrinsics", None)
        ups, lats = [p["pred_gravity_original"] for p in plist], [p["pred_latitude_original"] for p in plist]
        if shared is None or shared is False:
            res = fit_camera_params(ups, lats, **kw)
        else:  # True: one camera; otherwise one label per image
            res = fit_camera_shared(ups, lats, None if shared is True else shared, **kw)
        return res[0] if single else res

    def field_errors(self, preds, up_gt, lat_gt, **kw):
        """Errors of the dense fields of one inference() result (a dict) or of an inference_batch() list against ground-truth
        fields (e.g. crop_panorama's labels), on the GPU; see field_errors for the options and the returned entries."""
        single = isinstance(preds, dict)
        plist = [preds] if single else list(preds)
        ups, lats = [p["pred_gravity_original"] for p in plist], [p["pred_latitude_original"] for p in plist]
        return field_errors(ups[0], lats[0], up_gt, lat_gt, **kw) if single else field_errors(ups, lats, up_gt, lat_gt, **kw)

    def placement_scores(self, pred_bg, pred_obj, **kw):
        """The Perspective Field Discrepancy of pasting the picture of `pred_obj` onto the picture of `pred_bg` at every offset, on the GPU, from
        the dense fields of inference* results: one result dict each, or lists of them (every background against every object unless `pairs` says
        otherwise); see placement_scores for the options -- mask, stride, pairs, min_valid, weights -- and the returned entries."""
        def fields(preds):
            single = isinstance(preds, dict)
            plist = [preds] if single else list(preds)
            ups, lats = [p["pred_gravity_original"] for p in plist], [p["pred_latitude_original"] for p in plist]
            return (ups[0], lats[0]) if single else (ups, lats)

        return placement_scores(*fields(pred_bg), *fields(pred_obj), **kw)

    def placement_search(self, pred_bg, pred_obj, **kw):
        """placement_scores' arguments, searched over sizes and in-plane tilts of the object on the GPU: where, how large and how tilted the picture
        of `pred_obj` fits the picture of `pred_bg` best; see placement_search for the options -- scales, rotations, mask, stride, pairs, min_valid,
        weights, return_maps -- and the returned entries."""
        def fields(preds):
            single = isinstance(preds, dict)
            plist = [preds] if single else list(preds)
            ups, lats = [p["pred_gravity_original"] for p in plist], [p["pred_latitude_original"] for p in plist]
            return (ups[0], lats[0]) if single else (ups, lats)

        return placement_search(*fields(pred_bg), *fields(pred_obj), **kw)

    def composite(self, images_bg, images_obj, search, *, alpha=None, **kw):
        """The pictures of a placement search pasted where the search put them, on the GPU: `search` is what placement_search / m.placement_search
        returned (one dict, or the list with one dict per pair), images_bg and images_obj are the pictures whose fields were searched, of the
        fields' sizes and in the arrangement the search took them in.  best_scale, best_rotation_deg, best_offset and best_size go into
        composite_objects as the device tensors they are, so nothing is read back between search and paste; a pair for which nothing fitted
        (best_variant -1) returns its background.  alpha: the objects' masks or mattes; see composite_objects for it and for the options --
        pairs (the pairs the search was given), opacity, edge, samples, return_coverage -- and what is returned."""
        res = [search] if isinstance(search, dict) else list(search)
        if not res or not all(isinstance(d, dict) and {"best_scale", "best_rotation_deg", "best_offset", "best_size", "best_variant"} <= set(d) for d in res):
            raise ValueError("composite: search must be the result of placement_search: a dict or a list of dicts with best_scale, best_rotation_deg, "
                             "best_offset, best_size and best_variant")
        nan = float("nan")
        found = [d["best_variant"] >= 0 for d in res]
        col = lambda key, i=None: torch.stack([torch.where(f, (d[key] if i is None else d[key][i]).to(torch.float64), torch.full_like(d["best_scale"], nan))
                                               for d, f in zip(res, found)])
        return composite_objects(images_bg, images_obj, scale=col("best_scale"), rotation=col("best_rotation_deg"),
                                 offset=torch.stack([col("best_offset", 0), col("best_offset", 1)], 1),
                                 size=torch.stack([col("best_size", 0), col("best_size", 1)], 1), alpha=alpha, **kw)

    def draw_fields(self, images, preds, **kw):
        """The dense fields of inference* results drawn over their pictures, on the GPU: one result dict for one image, or a list of them for a
        list of images or a (B, H, W, 3) tensor; see draw_perspective_fields for `images`, the options -- density, arrow_inv_len, lat_step_deg,
        alpha, arrow_color, line_width, draw_up, draw_lat, out -- and what is returned.  The pictures are device tensors of the results' sizes, in
        the channel order they are to be shown in."""
        single = isinstance(preds, dict)
        plist = [preds] if single else list(preds)
        ups, lats = [p["pred_gravity_original"] for p in plist], [p["pred_latitude_original"] for p in plist]
        return draw_perspective_fields(images, ups[0] if single else ups, lats[0] if single else lats, **kw)

    @staticmethod
    def _pred_cameras(fn, preds):
        """the cameras of inference* / fit_camera results as a dict of one column per parameter (degrees), on the device where the results hold tensors"""
        plist = [preds] if isinstance(preds, dict) else list(preds)
        if not plist:
            raise ValueError(f"{fn} needs at least one result dict")
        for p in plist:
            if any(k not in p for k in ("pred_roll", "pred_pitch", "pred_rel_focal")):
                raise PfError(f"{fn} needs camera parameters (pred_roll, pred_pitch, pred_rel_focal) and this result has none: a PersNet "
                              "model predicts fields only; pass the result of fit_camera(preds) instead")

        def column(key):  # one value per result
            vals = [p.get(key, 0.0) for p in plist]
            tens = [v for v in vals if torch.is_tensor(v)]
            if not tens:
                return np.asarray(vals, dtype=np.float64)
            return torch.stack([v.reshape(()).to(device=tens[0].device, dtype=torch.float64) if torch.is_tensor(v)
                                else torch.tensor(float(v), dtype=torch.float64, device=tens[0].device) for v in vals])

        return {k: column("pred_" + k) for k in ("roll", "pitch", "rel_focal", "rel_cx", "rel_cy", "xi")}

    def rectify(self, images, preds, *, level="roll", undistort=True, rel_focal=None, height=None, width=None, **kw):
        """The images warped with their recovered cameras, on the GPU (see reproject_image for `images`, the other options --
        src_index, fill, return_valid, return_map, samples -- and what is returned).  preds: one result dict, or a list of them, of inference*
        (a ParamNet model) or of fit_camera; the source camera is pred_roll, pred_pitch, pred_rel_focal, pred_rel_cx, pred_rel_cy and
        pred_xi (absent keys count as 0), one per image (or per src_index entry).
        level: "roll" -- the destination camera has roll 0 and the source's pitch (an upright view); "full" -- roll 0 and pitch 0 (the
        horizon through the centre); "none" -- both kept.  The destination is always centred (rel_cx = rel_cy = 0).  undistort=True
        gives it xi = 0 (a pinhole view), False keeps the source's xi.  rel_focal: its focal length (in heights of the output), default the
        source's.  height, width: the output size, default the images'.
        The perspective fields of the rectified view are `fields_from_params` of the destination camera (roll, pitch, rel_focal, 0, 0, xi
        as stated here); they need no network."""
        if level not in ("roll", "full", "none"):
            raise ValueError("level must be 'roll', 'full' or 'none'")
        if "mode" in kw:
            raise ValueError("rectify takes the angles of its preds, which are degrees: no mode")
        src = PerspectiveFields._pred_cameras("rectify", preds)
        dst = dict(roll=src["roll"] if level == "none" else 0.0, pitch=0.0 if level == "full" else src["pitch"],
                   rel_focal=src["rel_focal"] if rel_focal is None else rel_focal, xi=0.0 if undistort else src["xi"])
        return reproject_image(images, src, dst, height=height, width=width, mode="deg", **kw)

    def compose_panorama(self, images, preds, *, yaw=0.0, **kw):
        """The images placed on equirectangular panoramas with their recovered cameras, on the GPU (see compose_panorama for `images`, the
        options -- height, width, pano_index, n_pano, blend, fill, return_weight -- and what is returned).  preds: one result dict, or a
        list of them, of inference* (a ParamNet model) or of fit_camera, one per image, read as `rectify` reads them.  The fields say nothing
        about the direction a view faces, so yaw (degrees; a number or one per image) is the caller's."""
        if "mode" in kw:
            raise ValueError("compose_panorama takes the angles of its preds, which are degrees: no mode")
        cams = PerspectiveFields._pred_cameras("compose_panorama", preds)
        cams["yaw"] = yaw
        return compose_panorama(images, cams, mode="deg", **kw)

    def align_yaw(self, images, preds, **kw):
        """The yaw of every image, recovered from the pictures with the cameras of `preds`, on the GPU (see align_yaw for the options -- anchor,
        step, stride, min_overlap, min_score, refine, return_info -- and what is returned).  preds: a list of result dicts of inference* (a
        ParamNet model) or of fit_camera, one per image, read as `rectify` reads them.  The result is what `compose_panorama` takes as `yaw`."""
        if "mode" in kw:
            raise ValueError("align_yaw takes the angles of its preds, which are degrees: no mode")
        return align_yaw(images, PerspectiveFields._pred_cameras("align_yaw", preds), mode="deg", **kw)

    def level_panorama(self, pano, *, n_yaw=8, view_pitch=(0.0,), vfov=90.0, view_size=None, use="paramnet", return_info=False, preds=None, samples=1):
        """A tilted equirectangular panorama made upright, on the GPU: n_yaw x len(view_pitch) square pinhole views of `vfov` degrees are cut out of it
        (crop_panorama: yaw k 360 / n_yaw, the pitches of view_pitch in degrees, roll 0, view_size pixels, default the network's input size), the model
        predicts every view's roll and pitch, `gravity_from_views` turns them into the panorama's roll and pitch, and
        `rotate_panorama(pano, roll, pitch, inverse=True)` re-samples it.
        pano: one CUDA tensor (H, W, 3), uint8 or float32 (on the 0 .. 255 scale; the views go to the network as uint8).
        use: "paramnet" -- the ParamNet scalars pred_roll / pred_pitch of every view; "fit" -- `fit_camera` on every view's dense fields (the only
        choice for a PersNet model).
        samples: the antialiasing of both steps, 1 .. 4 (crop_panorama's and rotate_panorama's `samples`); the views shrink a large panorama a lot.
        preds: the per-view results, one dict per view in the order pitch-major, yaw-minor -- inference results, or dicts with pred_roll / pred_pitch
        ("paramnet") or pred_gravity_original / pred_latitude_original ("fit"); given, nothing is cropped and the network does not run.
        Returns the upright panorama (H, W, 3) in the source's dtype; with return_info=True also a dict: roll, pitch (the estimate, degrees), views
        (the views' roll, pitch, yaw), preds (one per view, after the fit with use="fit") and gravity (gravity_from_views' result)."""
        if use not in ("paramnet", "fit"):
            raise ValueError("use must be 'paramnet' or 'fit'")
        samples = _check_samples("level_panorama", samples)
        n_yaw = operator.index(n_yaw)
        pitches = [float(v) for v in (view_pitch if isinstance(view_pitch, (list, tuple)) else [view_pitch])]
        if n_yaw < 1 or not pitches:
            raise ValueError("level_panorama needs n_yaw >= 1 and at least one view pitch")
        if not (0.0 < float(vfov) < 180.0):
            raise ValueError("vfov must be in (0, 180) degrees")
        size = NET_H if view_size is None else int(view_size)
        if size < 8:
            raise ValueError("view_size must be at least 8")
        if not torch.is_tensor(pano):
            raise TypeError("level_panorama takes one panorama, a torch tensor (H, W, 3)")
        _cuda_image_list("level_panorama", [pano], ("panorama", "panoramas"), "a panorama must be (H, W, 3) with H, W >= 2", 2)
        views = {"roll": [0.0] * (n_yaw * len(pitches)), "pitch": [p for p in pitches for _ in range(n_yaw)],
                 "yaw": [k * 360.0 / n_yaw for _ in pitches for k in range(n_yaw)]}
        n = n_yaw * len(pitches)
        if preds is None:
            crops = crop_panorama(pano, 0.0, views["pitch"], 0.5 / math.tan(math.radians(float(vfov)) / 2), yaw=views["yaw"], height=size, width=size, fields=False,
                                  samples=samples)[0]
            if crops.dtype != torch.uint8:
                crops = crops.round().clamp(0, 255).to(torch.uint8)
            preds = self.inference_batch(list(crops))
        else:
            preds = [preds] if isinstance(preds, dict) else list(preds)
            if len(preds) != n:
                raise ValueError(f"level_panorama: {len(preds)} preds for {n} views")
        if use == "fit":
            preds = self.fit_camera(preds)
        cams = PerspectiveFields._pred_cameras("level_panorama", preds)
        est = gravity_from_views(views, cams["roll"], cams["pitch"], mode="deg")
        out = rotate_panorama(pano, est["roll"], est["pitch"], inverse=True, mode="deg", samples=samples)[0]
        if not return_info:
            return out
        return out, {"roll": est["roll"], "pitch": est["pitch"], "views": views, "preds": preds, "gravity": est}

    def forward(self, batched_inputs) -> List[dict]:
        """batched_inputs: list of {"image": (3,320,320) float BGR 0..255, "height", "width"} (reference :223-272)."""
        with torch.no_grad():
            imgs = torch.stack([x["image"].to(self.device, dtype=torch.float32) for x in batched_inputs])
            sizes = [(int(x.get("height")), int(x.get("width"))) for x in batched_inputs]
            return self._run(imgs, sizes)

    # -------------------------------------------------------------------- engine path
    # images per engine forward: longer lists are processed in chunks (the reference accepts any list length; one
    # pf_forward call is limited to PF_MAX_BATCH = 81 images by its 32-bit activation offsets, include/pf_hip.h)
    MAX_CHUNK = 64

    def _run(self, batch, sizes, lazy_params=None, sat_out=None) -> List[dict]:
        """lazy_params: a list -> the ParamNet entries are NOT added to the result dicts here; (results of the chunk, raw (B,8) params) pairs are appended instead and
        the caller adds them once the parameters are complete (inference_stream with the deferred branch).  sat_out: a list -> the saturation watch of 'auto' is not
        read here (that would synchronise); (snapshot, batch, sizes, results) is appended for the caller to look at when the batch has finished."""
        eng = self._get_engine()
        chunk = max(1, min(int(os.environ.get("PF_MAX_CHUNK", self.MAX_CHUNK)), eng.max_batch))
        if len(sizes) > chunk:
            out: List[dict] = []
            for i0 in range(0, len(sizes), chunk):
                out.extend(self._run(batch[i0:i0 + chunk], sizes[i0:i0 + chunk], lazy_params, sat_out))
            return out
        if self.precision == "auto":  # first batch: look at the weights' static bounds and at the activations this checkpoint produces, then settle on a precision
            probe = batch if batch.dtype == torch.uint8 else batch.permute(0, 2, 3, 1).round().clamp(0, 255).to(torch.uint8)  # forward(): (B,3,320,320) float -> the u8 NHWC form of the debug entry
            _, _, _, _, rng = eng.forward_debug(probe.contiguous(), shadow=False, ranges=True)
            outside = [r for r in rng if r["saturated"] > 0 or r["max_abs"] > _window_limit(r) or r["non_finite"] > 0 or 0.0 < r["rms"] < 2.0 ** -5]
            static_max = eng.static_window_max()
            self.precision = "fp32_bf16x6" if (outside or static_max > 65504.0) else "fp32"
            if outside:
                self.precision_reason = (f"{len(outside)} of {len(rng)} dense-layer inputs outside the split-f16 window, first: {outside[0]['name']} "
                                         f"(max |x| {outside[0]['max_abs']:.4g}, rms {outside[0]['rms']:.4g})")
            elif static_max > 65504.0:
                self.precision_reason = f"a weights-only bound of an unwatched tensor (LayerNorm output / fused-MLP hidden map) reaches {static_max:.4g} > 65504"
            else:
                self.precision_reason = f"all {len(rng)} dense-layer inputs inside the split-f16 window (static bounds <= {static_max:.4g}); later batches are watched by the saturation counter"
            eng.set_precision(self.precision)
            eng.sat_seen = int(eng.saturation_snapshot())
        watch = self._auto and self.precision == "fp32"
        pg, pl, params = eng.forward(batch)
        snap = eng.saturation_snapshot() if watch else None
        results = self._assemble(eng, pg, pl, params, sizes, lazy_params)
        if watch:
            if sat_out is not None:
                sat_out.append((snap, batch, sizes, results))   # inference_stream looks when the batch is finished
            elif self._left_window(eng, snap):
                if lazy_params is not None and params is not None:
                    lazy_params.pop()
                results = self._rerun_exact(eng, batch, sizes, lazy_params)
        return results

    def _left_window(self, eng, snap) -> bool:
        """True when the forward behind `snap` moved the saturation counter (reading it synchronises with that forward)."""
        cnt = int(snap)
        moved = cnt != eng.sat_seen
        eng.sat_seen = cnt
        return moved

    def _rerun_exact(self, eng, batch, sizes, lazy_params=None):
        """Re-run of a batch that left the split-f16 window, in the exact mode (where the model then stays).  Always JOINED forwards: with the deferred ParamNet branch
        on, the branch is switched off around the re-run (which also puts the current stream behind a pending branch of a later batch), so that the scalar entries built
        right here read finished parameters; chunked like _run (a stream batch may exceed the engine's per-forward limit)."""
        import warnings

        if self.precision != "fp32_bf16x6":
            self.precision = "fp32_bf16x6"
            self.precision_reason = "a later batch left the split-f16 window (saturation counter moved): re-run and continuing in the exact bf16 split"
            warnings.warn("PerspectiveFields(precision='auto'): " + self.precision_reason)
            eng.set_precision(self.precision)
        deferred = bool(getattr(eng, "defer_params", False))
        if deferred:
            eng.set_defer_params(False)
        try:
            chunk = max(1, min(int(os.environ.get("PF_MAX_CHUNK", self.MAX_CHUNK)), eng.max_batch))
            out: List[dict] = []
            for i0 in range(0, len(sizes), chunk):
                pg, pl, params = eng.forward(batch[i0:i0 + chunk])
                out.extend(self._assemble(eng, pg, pl, params, sizes[i0:i0 + chunk], lazy_params))
        finally:
            if deferred:
                eng.set_defer_params(True)
        return out

    def _assemble(self, eng, pg, pl, params, sizes, lazy_params=None) -> List[dict]:
        results = []
        fields = eng.postprocess_batch(pg, pl, sizes)  # the reference's per-image post-process loop as one launch
        for i, (h, w) in enumerate(sizes):
            up, lat = fields[i]
            results.append(
                {
                    "pred_gravity": pg[i],
                    "pred_gravity_original": up,
                    "pred_latitude": pl[i],
                    "pred_latitude_original": lat,
                    "pred_latitude_original_mode": "deg",
                }
            )
        if params is not None:
            if lazy_params is not None:
                lazy_params.append((results, params))
            else:
                for i, extra in enumerate(self._param_dicts(params)):
                    results[i].update(extra)
        return results

    def _param_dicts(self, params) -> List[dict]:
        """(B,8) engine output -> the reference's per-image scalar dict entries
        (param_network.py:54-69 / 199-221 and perspectivefields.py:260-271)."""
        B = params.shape[0]
        if self.arch["param_net"] == "ParamNet":
            zeros = torch.zeros(B, dtype=torch.float32, device=params.device)
            cols = OrderedDict(
                pred_roll=params[:, 0], pred_pitch=params[:, 1], pred_vfov=params[:, 2], pred_rel_focal=params[:, 3],
                pred_general_vfov=params[:, 2], pred_rel_cx=zeros, pred_rel_cy=zeros,
            )
            return [{k: v[i] for k, v in cols.items()} for i in range(B)]
        # ParamNetConvNextRegress: factors per predicted parameter; rel_focal from general_vfov in closed form -- on the device for the zoo's output order (column 5 of the
        # engine's (B, 8) output, paramnet_scalars_kernel: no host round trip on the hot path), on the host for any other order of PREDICT_PARAMS
        factors = {"roll": 90.0, "pitch": 90.0, "vfov": 90.0, "rel_focal": 1.0, "rel_cx": 1.0, "rel_cy": 1.0, "general_vfov": 90.0}
        cols = OrderedDict()
        for j, key in enumerate(self.arch["predict_params"]):
            cols["pred_" + key] = params[:, j] * factors[key]
        if "pred_rel_focal" not in cols:
            if list(self.arch["predict_params"]) == list(self._DEVICE_FOCAL_ORDER):
                cols["pred_rel_focal"] = params[:, 5]
            else:
                cols["pred_rel_focal"] = torch.from_numpy(
                    general_vfov_to_focal(
                        cols["pred_rel_cx"].double().cpu().numpy(), cols["pred_rel_cy"].double().cpu().numpy(),
                        cols["pred_general_vfov"].double().cpu().numpy(),
                    ).astype(np.float32)
                )
        return [{k: v[i] for k, v in cols.items()} for i in range(B)]

    _DEVICE_FOCAL_ORDER = ("roll", "pitch", "general_vfov", "rel_cx", "rel_cy")   # every ParamNetConvNextRegress entry of the zoo (config/paramnet_*_rpfpp.yaml:32-37)


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
    import ctypes  # noqa: F401

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


# columns of the pf_fit_camera output row (include/pf_hip.h PF_FIT_COL_*)
_FIT_COLS = ("pred_roll", "pred_pitch", "pred_vfov", "pred_rel_focal", "pred_general_vfov", "pred_rel_cx", "pred_rel_cy",
             "fit_rms_up_deg", "fit_rms_lat_deg", "fit_cost", "fit_iterations", "fit_converged", "fit_valid_pixels")
_FIT_LOSSES = {"l2": 0, "huber": 1}
# columns of the pf_fit_camera_usm output row (PF_USMFIT_COL_*): the same, then xi
_USMFIT_COLS = _FIT_COLS + ("pred_xi",)


def _fit_init_rows(init, B, dev, distortion):
    """the `init` dicts of the camera fits -> None or a device [B][5 or 6] fp32 tensor of theta (angles in radians)"""
    if init is None:
        return None
    inits = [init] if isinstance(init, dict) else list(init)
    if len(inits) != B:
        raise ValueError(f"init has {len(inits)} entries for {B} images")
    rows = []
    for d in inits:
        z = torch.zeros((), dtype=torch.float64, device=dev)
        v = [torch.as_tensor(d[k], dtype=torch.float64).to(dev).reshape(()) for k in ("pred_roll", "pred_pitch", "pred_rel_focal")]
        v += [torch.as_tensor(d[k], dtype=torch.float64).to(dev).reshape(()) if k in d else z
              for k in ("pred_rel_cx", "pred_rel_cy") + (("pred_xi",) if distortion else ())]
        v[0], v[1] = torch.deg2rad(v[0]), torch.deg2rad(v[1])
        rows.append(torch.stack(v))
    return torch.stack(rows).to(torch.float32).contiguous()


def fit_camera_params(up, lat, *, free_principal_point=False, loss="l2", huber_delta_deg=2.0, weights=(1.0, 1.0), max_iter=20, init=None, distortion=False):
    """Perspective fields -> camera parameters on the GPU: the inverse of `fields_from_params`, a per-image Levenberg-Marquardt
    least-squares fit of its model to an up field (2,H,W) and a latitude map (H,W) in degrees (the layout of
    `pred_gravity_original` / `pred_latitude_original`).  Model, loss and stopping rule: include/pf_hip.h pf_fit_camera.

    up / lat: one pair of device tensors, or lists of pairs (sizes may differ; one launch sequence per 32 images).
    free_principal_point: fit rel_cx / rel_cy too (5 parameters); otherwise they stay at their start values (0 without `init`).
    loss: "l2" or "huber" (threshold huber_delta_deg); weights = (w_up, w_lat); max_iter: LM steps per image.
    init: optional start, one dict (or a list of dicts) with pred_roll, pred_pitch (degrees), pred_rel_focal and optionally
    pred_rel_cx / pred_rel_cy -- e.g. an inference() result of a ParamNet model.

    Returns one dict per image (a single dict for a single pair): pred_roll, pred_pitch, pred_vfov, pred_rel_focal,
    pred_general_vfov, pred_rel_cx, pred_rel_cy (angles in degrees), fit_rms_up_deg, fit_rms_lat_deg, fit_cost, fit_iterations,
    fit_converged, fit_valid_pixels -- 0-d device tensors (no host synchronisation), so `fields_from_params` can take the
    pred_* entries directly.  GPU only: CPU tensors raise PfError.

    distortion=True fits the Unified Spherical Model of crop_panorama(..., xi=) instead (include/pf_hip.h pf_fit_camera_usm): the
    mirror parameter xi is free too -- 4 parameters, 6 with free_principal_point -- clamped to [-0.5, 2], and each dict gains `pred_xi`.
    `init` dicts may carry `pred_xi` (default 0); without `init` the start is the pinhole one at xi = 0, which recovers xi <= 1; for
    xi > 1 (part of the image has no ray) give a start.  pred_vfov / pred_general_vfov keep their formulas in rel_focal, rel_cx and
    rel_cy: under xi != 0 they describe the intrinsics, not the angle the image subtends.  fit_valid_pixels counts the pixels with finite
    input and a ray.  `fields_from_params(..., xi=d["pred_xi"])` turns a result back into fields.  distortion=False is the pinhole fit,
    unchanged."""
    from .engine import _check, _stream_ptr, load_library

    single = torch.is_tensor(up)
    ups, lats = ([up], [lat]) if single else (list(up), list(lat))
    if len(ups) != len(lats) or not ups:
        raise ValueError("fit_camera_params needs as many latitude maps as up fields, at least one")
    if loss not in _FIT_LOSSES:
        raise ValueError(f"loss must be one of {sorted(_FIT_LOSSES)}")
    for u, l in zip(ups, lats):
        if not (torch.is_tensor(u) and torch.is_tensor(l)):
            raise TypeError("fit_camera_params takes torch tensors")
        if not (u.is_cuda and l.is_cuda):
            raise PfError("fit_camera_params runs on the GPU only (no CPU path)")
        if u.dim() != 3 or u.shape[0] != 2 or tuple(l.shape) != tuple(u.shape[1:]):
            raise ValueError(f"up must be (2, H, W) and lat (H, W); got {tuple(u.shape)} and {tuple(l.shape)}")
    dev = ups[0].device
    if any(t.device != dev for t in ups + lats):
        raise ValueError("fit_camera_params: all fields must be on one device")
    ups = [u.to(torch.float32).contiguous() for u in ups]
    lats = [l.to(torch.float32).contiguous() for l in lats]
    B = len(ups)
    d_init = _fit_init_rows(init, B, dev, distortion)
    hw = (ctypes.c_int32 * (2 * B))(*[s for u in ups for s in (int(u.shape[1]), int(u.shape[2]))])
    p_up = (ctypes.c_void_p * B)(*[u.data_ptr() for u in ups])
    p_lat = (ctypes.c_void_p * B)(*[l.data_ptr() for l in lats])
    lib = load_library()
    entry, cols = ("pf_fit_camera_usm", _USMFIT_COLS) if distortion else ("pf_fit_camera", _FIT_COLS)
    ws_n = int(getattr(lib, entry + "_workspace_bytes")(B, hw))
    if ws_n == 0:
        small = [tuple(u.shape[1:]) for u in ups if min(u.shape[1:]) < 8]
        raise PfError(f"fit_camera_params: images must be at least 8 x 8 (got {small})")
    ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
    out = torch.empty((B, len(cols)), dtype=torch.float32, device=dev)
    w_up, w_lat = (float(w) for w in weights)
    with torch.cuda.device(dev):
        _check(getattr(lib, entry)(dev.index, B, hw, p_up, p_lat, d_init.data_ptr() if d_init is not None else None, int(bool(free_principal_point)),
                                   _FIT_LOSSES[loss], float(huber_delta_deg), w_up, w_lat, int(max_iter), out.data_ptr(), ws.data_ptr(), ws_n,
                                   _stream_ptr()), None, entry)
    iters = out[:, 10].to(torch.int32)
    conv = out[:, 11] != 0
    valid = out[:, 12].to(torch.int64)
    res = []
    for i in range(B):
        d = {k: out[i, j] for j, k in enumerate(_FIT_COLS[:10])}
        d["fit_iterations"], d["fit_converged"], d["fit_valid_pixels"] = iters[i], conv[i], valid[i]
        if distortion:
            d["pred_xi"] = out[i, 13]
        res.append(d)
    return res[0] if single else res


def fit_camera_shared(up, lat, groups=None, *, distortion=False, free_principal_point=False, loss="l2", huber_delta_deg=2.0, weights=(1.0, 1.0), max_iter=20,
                      init=None):
    """The camera fit of `fit_camera_params` for images that share a camera -- the frames of a video, a photo set of one device: every
    image keeps its own roll and pitch, all images of a group share rel_focal, with free_principal_point also rel_cx / rel_cy, with
    distortion=True also xi.  One joint Levenberg-Marquardt fit per group on the GPU (include/pf_hip.h pf_fit_camera_shared).

    up / lat: lists of device tensors (2,H,W) / (H,W), as for fit_camera_params.  groups: None -- all images are one camera -- or one hashable
    label per image, in any order; the images of a group must have one size (rel_focal is relative to the height), groups may differ.
    The other options are those of fit_camera_params; `init` gives every image's start, the group starts from its images' mean.

    Returns one dict per image, in the caller's order, with the entries of fit_camera_params: the image's own pred_roll, pred_pitch,
    fit_rms_*, fit_cost and fit_valid_pixels; the group's pred_rel_focal, pred_rel_cx, pred_rel_cy, pred_xi (the same bits in every dict
    of a group), fit_iterations and fit_converged; plus fit_group_cost (0-d device tensor: the group's summed cost) and fit_group (the
    label; 0 with groups=None).  An image without a valid pixel contributes nothing: fit_valid_pixels 0, fit_converged False.
    GPU only: CPU tensors raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    if torch.is_tensor(up) or torch.is_tensor(lat):
        raise TypeError("fit_camera_shared takes lists of fields, one pair per image")
    ups, lats = list(up), list(lat)
    if len(ups) != len(lats) or not ups:
        raise ValueError("fit_camera_shared needs as many latitude maps as up fields, at least one")
    if loss not in _FIT_LOSSES:
        raise ValueError(f"loss must be one of {sorted(_FIT_LOSSES)}")
    B = len(ups)
    labels = [0] * B if groups is None else list(groups)
    if len(labels) != B:
        raise ValueError(f"groups has {len(labels)} labels for {B} images")
    for u, l in zip(ups, lats):
        if not (torch.is_tensor(u) and torch.is_tensor(l)):
            raise TypeError("fit_camera_shared takes torch tensors")
        if u.dim() != 3 or u.shape[0] != 2 or tuple(l.shape) != tuple(u.shape[1:]):
            raise ValueError(f"up must be (2, H, W) and lat (H, W); got {tuple(u.shape)} and {tuple(l.shape)}")
    members = {}   # label -> its images, in the caller's order; the groups in the order of their first image
    for i, g in enumerate(labels):
        members.setdefault(g, []).append(i)
    for g, idx in members.items():
        sizes = sorted({tuple(ups[i].shape[1:]) for i in idx})
        if len(sizes) > 1:
            raise ValueError(f"fit_camera_shared: the images of group {g!r} have different sizes {sizes}; a camera group needs one size")
    if not all(u.is_cuda and l.is_cuda for u, l in zip(ups, lats)):
        raise PfError("fit_camera_shared runs on the GPU only (no CPU path)")
    dev = ups[0].device
    if any(t.device != dev for t in ups + lats):
        raise ValueError("fit_camera_shared: all fields must be on one device")
    order = [i for idx in members.values() for i in idx]   # consecutive groups
    ups = [ups[i].to(torch.float32).contiguous() for i in order]
    lats = [lats[i].to(torch.float32).contiguous() for i in order]
    if init is not None and not isinstance(init, dict):
        init = list(init)
        if len(init) != B:
            raise ValueError(f"init has {len(init)} entries for {B} images")
        init = [init[i] for i in order]
    d_init = _fit_init_rows(init, B, dev, distortion)
    hw = (ctypes.c_int32 * (2 * B))(*[s for u in ups for s in (int(u.shape[1]), int(u.shape[2]))])
    gs = (ctypes.c_int32 * len(members))(*[len(idx) for idx in members.values()])
    p_up = (ctypes.c_void_p * B)(*[u.data_ptr() for u in ups])
    p_lat = (ctypes.c_void_p * B)(*[l.data_ptr() for l in lats])
    lib = load_library()
    model, cols = (1, _USMFIT_COLS) if distortion else (0, _FIT_COLS)
    ws_n = int(lib.pf_fit_camera_shared_workspace_bytes(model, B, hw, len(members), gs))
    if ws_n == 0:
        small = [tuple(u.shape[1:]) for u in ups if min(u.shape[1:]) < 8]
        raise PfError(f"fit_camera_shared: images must be at least 8 x 8 (got {small})")
    ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
    out = torch.empty((B, len(cols)), dtype=torch.float32, device=dev)
    w_up, w_lat = (float(w) for w in weights)
    with torch.cuda.device(dev):
        _check(lib.pf_fit_camera_shared(dev.index, model, B, hw, p_up, p_lat, len(members), gs, d_init.data_ptr() if d_init is not None else None,
                                        int(bool(free_principal_point)), _FIT_LOSSES[loss], float(huber_delta_deg), w_up, w_lat, int(max_iter),
                                        out.data_ptr(), ws.data_ptr(), ws_n, _stream_ptr()), None, "pf_fit_camera_shared")
    iters = out[:, 10].to(torch.int32)
    conv = out[:, 11] != 0
    valid = out[:, 12].to(torch.int64)
    res = [None] * B
    row = 0
    for g, idx in members.items():
        group_cost = out[row:row + len(idx), 9].to(torch.float64).sum()
        for i in idx:
            d = {k: out[row, j] for j, k in enumerate(_FIT_COLS[:10])}
            d["fit_iterations"], d["fit_converged"], d["fit_valid_pixels"] = iters[row], conv[row], valid[row]
            if distortion:
                d["pred_xi"] = out[row, 13]
            d["fit_group_cost"], d["fit_group"] = group_cost, g
            res[i] = d
            row += 1
    return res


# columns of the pf_field_errors output row (include/pf_hip.h PF_FERR_COL_*), bins and running totals of its histogram (PF_FERR_BINS, PF_FERR_SUM_*)
_FERR_COLS = ("up_mean_deg", "up_median_deg", "up_rmse_deg", "up_max_deg", "up_frac_below",
              "lat_mean_deg", "lat_median_deg", "lat_rmse_deg", "lat_max_deg", "lat_frac_below", "valid_pixels")
_FERR_BINS, _FERR_BINS_PER_DEG = 11520, 64
_FERR_SUMS = ("n", "sum", "sum_sq", "max", "below")


def _field_list(what, up, lat, fn="field_errors"):
    """one (2,H,W) / (H,W) pair, a batched (B,2,H,W) / (B,H,W) pair or lists of pairs -> (is a single pair, [up], [lat])"""
    if torch.is_tensor(up) != torch.is_tensor(lat):
        raise TypeError(f"{fn}: {what} up field and latitude must both be tensors or both be lists")
    if torch.is_tensor(up):
        if up.dim() == 4 and lat.dim() == 3:
            if up.shape[0] != lat.shape[0]:
                raise ValueError(f"{fn}: {what} up {tuple(up.shape)} and latitude {tuple(lat.shape)} differ in batch size")
            return False, list(up.unbind(0)), list(lat.unbind(0))
        return True, [up], [lat]
    if not isinstance(up, (list, tuple)) or not isinstance(lat, (list, tuple)):
        raise TypeError(f"{fn} takes torch tensors or lists of them")
    ups, lats = list(up), list(lat)
    if len(ups) != len(lats):
        raise ValueError(f"{fn}: {len(ups)} {what} up fields for {len(lats)} latitude maps")
    return False, ups, lats


def _field_errors(up_pred, lat_pred, up_gt, lat_gt, threshold_deg, return_maps, hist=None, sums=None):
    from .engine import _check, _stream_ptr, load_library

    s_p, ups_p, lats_p = _field_list("predicted", up_pred, lat_pred)
    s_g, ups_g, lats_g = _field_list("ground-truth", up_gt, lat_gt)
    if len(ups_p) != len(ups_g) or not ups_p:
        raise ValueError(f"field_errors needs as many ground-truth fields as predictions, at least one (got {len(ups_p)} and {len(ups_g)})")
    threshold_deg = float(threshold_deg)
    if not (threshold_deg > 0.0 and np.isfinite(threshold_deg)):
        raise ValueError("threshold_deg must be finite and > 0")
    every = ups_p + lats_p + ups_g + lats_g
    if not all(torch.is_tensor(t) for t in every):
        raise TypeError("field_errors takes torch tensors")
    for u, l, g, m in zip(ups_p, lats_p, ups_g, lats_g):
        if u.dim() != 3 or u.shape[0] != 2 or min(u.shape[1:]) < 1 or tuple(l.shape) != tuple(u.shape[1:]):
            raise ValueError(f"up must be (2, H, W) and lat (H, W) with H, W >= 1; got {tuple(u.shape)} and {tuple(l.shape)}")
        if tuple(g.shape) != tuple(u.shape) or tuple(m.shape) != tuple(l.shape):
            raise ValueError(f"ground truth {tuple(g.shape)} / {tuple(m.shape)} does not match the prediction {tuple(u.shape)} / {tuple(l.shape)}")
    if not all(t.is_cuda for t in every):
        raise PfError("field_errors runs on the GPU only (no CPU path)")
    dev = every[0].device
    if any(t.device != dev for t in every):
        raise ValueError("field_errors: all fields must be on one device")
    ups_p, lats_p, ups_g, lats_g = ([t.to(torch.float32).contiguous() for t in ts] for ts in (ups_p, lats_p, ups_g, lats_g))
    B = len(ups_p)
    ptrs = lambda ts: (ctypes.c_void_p * B)(*[t.data_ptr() for t in ts])
    hw = (ctypes.c_int32 * (2 * B))(*[s for u in ups_p for s in (int(u.shape[1]), int(u.shape[2]))])
    lib = load_library()
    ws_n = int(lib.pf_field_errors_workspace_bytes(B, hw))
    if ws_n == 0:
        raise PfError(f"field_errors: unsupported image sizes {[tuple(u.shape[1:]) for u in ups_p]}")
    ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
    out = torch.empty((B, len(_FERR_COLS)), dtype=torch.float64, device=dev)
    maps_up = [torch.empty_like(l) for l in lats_p] if return_maps else None
    maps_lat = [torch.empty_like(l) for l in lats_p] if return_maps else None
    with torch.cuda.device(dev):
        _check(lib.pf_field_errors(dev.index, B, hw, ptrs(ups_p), ptrs(lats_p), ptrs(ups_g), ptrs(lats_g), threshold_deg, out.data_ptr(),
                                   ptrs(maps_up) if return_maps else None, ptrs(maps_lat) if return_maps else None,
                                   hist.data_ptr() if hist is not None else None, sums.data_ptr() if sums is not None else None,
                                   ws.data_ptr(), ws_n, _stream_ptr()), None, "pf_field_errors")
    valid = out[:, len(_FERR_COLS) - 1].to(torch.int64)
    res = []
    valid = valid.unbind(0)
    for i, row in enumerate(out.unbind(0)):
        d = dict(zip(_FERR_COLS[:-1], row.unbind(0)))
        d["valid_pixels"] = valid[i]
        if return_maps:
            d["up_error_deg"], d["lat_error_deg"] = maps_up[i], maps_lat[i]
        res.append(d)
    return res[0] if (s_p and s_g) else res


def field_errors(up_pred, lat_pred, up_gt, lat_gt, *, threshold_deg=5.0, return_maps=False):
    """Predicted perspective fields against ground truth on the GPU: the per-pixel numbers of the paper's tables.  Definitions:
    include/pf_hip.h pf_field_errors.  Per pixel e_up = atan2(|cross|, dot) of the two up vectors and
    e_lat = |lat_pred - lat_gt|, both in degrees; a pixel with a non-finite value in any of its six inputs, or an up vector shorter
    than 1e-6, enters no statistic (crop_panorama's NaN labels mask themselves; mask a pixel by writing NaN into its label).

    up_* (2,H,W) and lat_* (H,W) degrees (the layout of `pred_gravity_original` / `pred_latitude_original` and of crop_panorama's
    labels): one set of device tensors, batched (B,2,H,W) / (B,H,W) tensors, or lists (sizes may differ; one launch sequence per
    32 images).  Returns one dict per image (a single dict for a single set) of 0-d float64 device tensors (no host
    synchronisation): up_mean_deg, up_median_deg, up_rmse_deg, up_max_deg, up_frac_below (share of valid pixels with
    e < threshold_deg, strict), lat_* likewise, valid_pixels (int64); with return_maps also up_error_deg, lat_error_deg (H,W)
    fp32, NaN where invalid.  The median is numpy's, exact: an element (or the fp64 mean of the two middle elements) of the fp32
    error map.  No valid pixel: NaN statistics and valid_pixels = 0.  Deterministic; an image's numbers do not depend on the batch
    it is in.  GPU only: CPU tensors raise PfError."""
    return _field_errors(up_pred, lat_pred, up_gt, lat_gt, threshold_deg, return_maps)


def placement_scores(up_bg, lat_bg, up_obj, lat_obj, *, mask=None, stride=1, pairs=None, min_valid=0.5, weights=(1.0, 1.0)):
    """Perspective-aware compositing on the GPU: the Perspective Field Discrepancy (PFD) of an object cut from one picture against a background
    at every place it could be pasted -- the mean up-vector angle plus the mean latitude difference over the object's pixels; a low PFD is what
    people judge as "fits".  Definitions: include/pf_hip.h pf_place_scores.

    up_bg (2,H,W), lat_bg (H,W) and up_obj (2,h,w), lat_obj (h,w) in degrees with h <= H, w <= W (the layout of `pred_gravity_original` /
    `pred_latitude_original` and of crop_panorama's labels): one set of device tensors each, batched tensors, or lists (sizes may differ).  A
    pixel with a non-finite value or an up vector shorter than 1e-6 is invalid in its own field, and a pixel pair counts only where both are
    valid: a NaN latitude masks a pixel, a silhouette is NaN outside the object, a background padded with NaN lets the object hang over the
    border.  mask: a bool (h,w) tensor, or a list of one per object (None entries allowed), True on the object; applied as NaN on a copy of
    the object's latitude.  The placement (j, i) puts the object's corner on background pixel (j stride, i stride); there are
    P x Q = ((H - h) // stride + 1) x ((W - w) // stride + 1) of them.  pairs: (background, object) index pairs, default every combination,
    backgrounds outermost.
    Returns one dict per pair (a single dict when both sides are a single set) of device tensors, no host synchronisation:
    up_mean_deg, lat_mean_deg (P,Q) float64, the means over the valid pairs (NaN where there is none); pfd_deg (P,Q) float64 =
    weights[0] up_mean_deg + weights[1] lat_mean_deg, the paper's sum at the default (1, 1), +inf where fewer than min_valid x (valid pixels of
    the object) pairs are valid or the object has no valid pixel; valid_pixels (P,Q) int64; best_offset (2,) int64, (row, col) of the lowest
    PFD in background pixels, the first in row-major order, (-1, -1) when every placement is +inf; best_pfd_deg; stride.
    The fields of a resized crop are the resized fields: transform_fields resizes and turns them, and placement_search runs this function over a
    set of scales and rotations and finds the best of all on the device.  Deterministic; a pair's numbers do not depend on the other pairs.  GPU
    only: CPU tensors raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    fn = "placement_scores"
    s_b, ups_b, lats_b = _field_list("background", up_bg, lat_bg, fn)
    s_o, ups_o, lats_o = _field_list("object", up_obj, lat_obj, fn)
    if not ups_b or not ups_o:
        raise ValueError(f"{fn} needs at least one background and one object")
    every = ups_b + lats_b + ups_o + lats_o
    if not all(torch.is_tensor(t) for t in every):
        raise TypeError(f"{fn} takes torch tensors")
    for u, l in zip(ups_b + ups_o, lats_b + lats_o):
        if u.dim() != 3 or u.shape[0] != 2 or min(u.shape[1:]) < 1 or tuple(l.shape) != tuple(u.shape[1:]):
            raise ValueError(f"up must be (2, H, W) and lat (H, W) with H, W >= 1; got {tuple(u.shape)} and {tuple(l.shape)}")
    stride = operator.index(stride)
    if stride < 1:
        raise ValueError(f"stride must be at least 1; got {stride}")
    min_valid = float(min_valid)
    if not 0.0 <= min_valid <= 1.0:
        raise ValueError(f"min_valid must be in [0, 1]; got {min_valid}")
    w_up, w_lat = (float(v) for v in weights)
    if not (w_up >= 0.0 and w_lat >= 0.0 and np.isfinite(w_up) and np.isfinite(w_lat)):
        raise ValueError(f"weights must be two finite numbers >= 0; got {weights}")
    nb, no = len(ups_b), len(ups_o)
    if pairs is None:
        plist = [(b, o) for b in range(nb) for o in range(no)]
    else:
        plist = [(operator.index(b), operator.index(o)) for b, o in (pairs.tolist() if torch.is_tensor(pairs) else pairs)]
        if not plist:
            raise ValueError(f"{fn} needs at least one pair")
    single = s_b and s_o and len(plist) == 1
    for b, o in plist:
        if not (0 <= b < nb and 0 <= o < no):
            raise ValueError(f"a pair is (background, object) with indices in [0, {nb}) and [0, {no}); got ({b}, {o})")
        if ups_o[o].shape[1] > ups_b[b].shape[1] or ups_o[o].shape[2] > ups_b[b].shape[2]:
            raise ValueError(f"the object {tuple(ups_o[o].shape[1:])} is larger than its background {tuple(ups_b[b].shape[1:])}")
    masks = [None] * no if mask is None else [mask] if torch.is_tensor(mask) else list(mask)
    if len(masks) != no:
        raise ValueError(f"{len(masks)} masks for {no} objects")
    for m, l in zip(masks, lats_o):
        if m is not None and (not torch.is_tensor(m) or m.dtype != torch.bool or tuple(m.shape) != tuple(l.shape)):
            raise ValueError(f"a mask is a bool tensor of its object's size {tuple(l.shape)}")
    every += [m for m in masks if m is not None]
    if not all(t.is_cuda for t in every):
        raise PfError(f"{fn} runs on the GPU only (no CPU path)")
    dev = every[0].device
    if any(t.device != dev for t in every):
        raise ValueError(f"{fn}: all fields and masks must be on one device")
    ups_b, lats_b, ups_o, lats_o = ([t.to(torch.float32).contiguous() for t in ts] for ts in (ups_b, lats_b, ups_o, lats_o))
    lats_o = [l if m is None else torch.where(m, l, torch.full_like(l, float("nan"))) for l, m in zip(lats_o, masks)]
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    sizes = lambda ts: (ctypes.c_int32 * (2 * len(ts)))(*[s for u in ts for s in (int(u.shape[1]), int(u.shape[2]))])
    hw_b, hw_o = sizes(ups_b), sizes(ups_o)
    n_pair = len(plist)
    c_pairs = (ctypes.c_int32 * (2 * n_pair))(*[i for bo in plist for i in bo])
    dims = [((ups_b[b].shape[1] - ups_o[o].shape[1]) // stride + 1, (ups_b[b].shape[2] - ups_o[o].shape[2]) // stride + 1) for b, o in plist]
    lib = load_library()
    need = int(lib.pf_place_scores_workspace_bytes(nb, hw_b, no, hw_o, n_pair, c_pairs, stride))
    if need == 0:
        raise ValueError(f"{fn}: field sizes that one call does not take (2^31 pixels or more, or an object of more than 65535 x 1024 pixels)")
    out = torch.empty(3 * sum(P * Q for P, Q in dims), dtype=torch.float64, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib.pf_place_scores(dev.index, nb, ptrs(ups_b), ptrs(lats_b), hw_b, no, ptrs(ups_o), ptrs(lats_o), hw_o, n_pair, c_pairs, stride,
                                   out.data_ptr(), ws.data_ptr(), need, _stream_ptr()), None, "pf_place_scores")
    # the valid pixels of every object, by the kernel's rule in float32 (a * a + b * b rounds twice where the kernel's fmaf rounds once: the two can
    # differ only for a squared length within an ulp of 1e-12)
    obj_valid = []
    for u, l in zip(ups_o, lats_o):
        l2 = u[0] * u[0] + u[1] * u[1]
        obj_valid.append((torch.isfinite(l) & (l2 >= 1e-12) & torch.isfinite(l2)).sum().to(torch.float64))
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=dev)
    res, first = [], 0
    for (b, o), (P, Q) in zip(plist, dims):
        rec = out[first:first + 3 * P * Q].view(P, Q, 3)
        first += 3 * P * Q
        n = rec[..., 2]
        up_mean, lat_mean = rec[..., 0] / n, rec[..., 1] / n   # NaN where n = 0
        ok = (n >= min_valid * obj_valid[o]) & (n > 0)
        pfd = torch.where(ok, w_up * up_mean + w_lat * lat_mean, inf)
        best = pfd.min()
        flat = torch.where(pfd.reshape(-1) == best, torch.arange(P * Q, device=dev), P * Q).min()   # the first of equal minima
        at = torch.stack([torch.div(flat, Q, rounding_mode="floor"), flat % Q]) * stride
        res.append(dict(pfd_deg=pfd, up_mean_deg=up_mean, lat_mean_deg=lat_mean, valid_pixels=n.to(torch.int64),
                        best_offset=torch.where(torch.isfinite(best), at, torch.full_like(at, -1)), best_pfd_deg=best, stride=stride))
    return res[0] if single else res


def _variant_values(name, v, fn):
    """a scalar or a sequence of finite floats -> (is a scalar, [float])"""
    scalar = not isinstance(v, (list, tuple, np.ndarray)) and not (torch.is_tensor(v) and v.dim() > 0)
    vals = [float(v)] if scalar else [float(x) for x in (v.tolist() if torch.is_tensor(v) or isinstance(v, np.ndarray) else v)]
    if not vals:
        raise ValueError(f"{fn}: {name} is empty")
    if not all(np.isfinite(x) for x in vals) or (name.startswith("scale") and not all(x > 0.0 for x in vals)):
        raise ValueError(f"{fn}: {name} must be finite{' and > 0' if name.startswith('scale') else ''}; got {vals}")
    return scalar, vals


def _masked_latitudes(lats, mask, what, fn):
    """the checks of mask= and the masks as a list, one per field (None entries allowed)"""
    masks = [None] * len(lats) if mask is None else [mask] if torch.is_tensor(mask) else list(mask)
    if len(masks) != len(lats):
        raise ValueError(f"{fn}: {len(masks)} masks for {len(lats)} {what}")
    for m, l in zip(masks, lats):
        if m is not None and (not torch.is_tensor(m) or m.dtype != torch.bool or tuple(m.shape) != tuple(l.shape)):
            raise ValueError(f"{fn}: a mask is a bool tensor of its field's size {tuple(l.shape)}")
    return masks


def transform_fields(up, lat, *, scale=1.0, rotation=0.0, mask=None, height=None, width=None):
    """The perspective fields of a picture that is resized by `scale` and turned by `rotation` degrees in its plane, on the GPU: the field-aware
    resample that an image resize is not -- NaN is the mask and must not spread, up vectors are mixed as vectors and made unit again, and a rotation
    turns the vectors with the picture.  Definitions: include/pf_hip.h pf_fields_transform.

    up (2,h,w), lat (h,w) in degrees (the layout of `pred_gravity_original` / `pred_latitude_original`): one field of device tensors, a batched
    pair, or lists.  scale > 0; rotation in degrees, positive = clockwise on the screen, the fields of a camera whose roll is lower by that much.
    Both are scalars or sequences of one length: a sequence gives a list of (up', lat'), one per variant.  The output is
    h' = max(1, floor(scale (h |cos| + w |sin|) + 1/2)) high, w' likewise with h and w exchanged, unless height= / width= say otherwise; the picture's
    centre stays the centre.  Four bilinear taps per pixel; a tap outside the array or on an invalid pixel (a non-finite value, an up vector shorter
    than 1e-6) is dropped, and the pixel is valid where the taps left carry at least half of the weight: NaN in all three planes otherwise.  So a
    silhouette keeps its outline to half a pixel and the array border behaves like a clamp.  There is no prefilter: fields are smooth, and only a
    silhouette aliases when scale is far below 1.  mask: a bool (h,w) tensor (or one per field), True inside; applied as NaN on a copy of the latitude.
    scale=1, rotation=0 returns the bits of a field of unit up vectors.  Returns (up', lat') float32 device tensors, a list of them for sequences, a
    list per field for several fields; no host synchronisation.  Deterministic; a variant's bits do not depend on the others.  GPU only: CPU
    tensors raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    fn = "transform_fields"
    single, ups, lats = _field_list("source", up, lat, fn)
    if not ups:
        raise ValueError(f"{fn} needs at least one field")
    if not all(torch.is_tensor(t) for t in ups + lats):
        raise TypeError(f"{fn} takes torch tensors")
    for u, l in zip(ups, lats):
        if u.dim() != 3 or u.shape[0] != 2 or min(u.shape[1:]) < 1 or tuple(l.shape) != tuple(u.shape[1:]):
            raise ValueError(f"up must be (2, h, w) and lat (h, w) with h, w >= 1; got {tuple(u.shape)} and {tuple(l.shape)}")
    s_scalar, scales = _variant_values("scale", scale, fn)
    r_scalar, rots = _variant_values("rotation", rotation, fn)
    if s_scalar != r_scalar:
        scales, rots = (scales * len(rots), rots) if s_scalar else (scales, rots * len(scales))
    if len(scales) != len(rots):
        raise ValueError(f"{fn}: {len(scales)} scales for {len(rots)} rotations")
    size = [None if v is None else operator.index(v) for v in (height, width)]
    if any(v is not None and v < 1 for v in size):
        raise ValueError(f"{fn}: height and width must be at least 1; got {height}, {width}")
    masks = _masked_latitudes(lats, mask, "fields", fn)
    every = ups + lats + [m for m in masks if m is not None]
    if not all(t.is_cuda for t in every):
        raise PfError(f"{fn} runs on the GPU only (no CPU path)")
    dev = every[0].device
    if any(t.device != dev for t in every):
        raise ValueError(f"{fn}: all fields and masks must be on one device")
    ups, lats = ([t.to(torch.float32).contiguous() for t in ts] for ts in (ups, lats))
    lats = [l if m is None else torch.where(m, l, torch.full_like(l, float("nan"))) for l, m in zip(lats, masks)]
    lib = load_library()
    jobs, outs = [], []
    for u, l in zip(ups, lats):
        res = []
        for s, r in zip(scales, rots):
            hw = (ctypes.c_int32 * 2)()
            if lib.pf_fields_transform_size(int(u.shape[1]), int(u.shape[2]), s, r, hw) != 0:
                raise ValueError(f"{fn}: {lib.pf_last_error(None).decode()}")
            ho, wo = (hw[0] if size[0] is None else size[0]), (hw[1] if size[1] is None else size[1])
            if ho * wo >= 2 ** 31:
                raise ValueError(f"{fn}: an output of {ho} x {wo} has 2^31 pixels or more")
            o_up, o_lat = torch.empty((2, ho, wo), dtype=torch.float32, device=dev), torch.empty((ho, wo), dtype=torch.float32, device=dev)
            jobs.append((u, l, s, r, ho, wo, o_up, o_lat))
            res.append((o_up, o_lat))
        outs.append(res[0] if s_scalar and r_scalar else res)
    n = len(jobs)
    ptrs = lambda k: (ctypes.c_void_p * n)(*[j[k].data_ptr() for j in jobs])
    c_hw = (ctypes.c_int32 * (2 * n))(*[v for j in jobs for v in (int(j[0].shape[1]), int(j[0].shape[2]))])
    c_var = (ctypes.c_double * (2 * n))(*[v for j in jobs for v in (j[2], j[3])])
    c_out = (ctypes.c_int32 * (2 * n))(*[v for j in jobs for v in (j[4], j[5])])
    with torch.cuda.device(dev):
        _check(lib.pf_fields_transform(dev.index, n, ptrs(0), ptrs(1), c_hw, c_var, c_out, ptrs(6), ptrs(7), _stream_ptr()), None, "pf_fields_transform")
    return outs[0] if single else outs


def placement_search(up_bg, lat_bg, up_obj, lat_obj, *, scales=(1.0,), rotations=(0.0,), mask=None, stride=1, pairs=None, min_valid=0.5, weights=(1.0, 1.0),
                     return_maps=False):
    """placement_scores over a set of sizes and in-plane tilts of the object, and the best of all of them found on the GPU: where, how large and how
    tilted the object fits its background best.  Definitions: include/pf_hip.h pf_place_search.

    The fields, mask, stride, pairs, min_valid and weights are placement_scores'; an object larger than its background is no error here.  The
    variants are the product scales x rotations, scales outermost: variant v = (scales[v // R], rotations[v % R]).  Each object is transformed by each
    variant (transform_fields, the mask applied first) and scored at every offset; min_valid counts against the valid pixels of the transformed
    object.  A variant whose transformed object does not fit its background is skipped: +inf, offset (-1, -1).
    Returns one dict per pair (a single dict under placement_scores' rule) of device tensors, no host synchronisation:
    best_scale, best_rotation_deg (float64, NaN when every placement of every variant is +inf), best_variant (int64, -1 then), best_offset (2,) int64
    (row, col) in background pixels, best_pfd_deg, best_up_mean_deg, best_lat_mean_deg, best_size (2,) int64 (h', w' of the best variant, (-1, -1)
    without one); variant_pfd_deg (V,), variant_offset (V,2), variant_size (V,2), variant_valid_pixels (V,); stride.  Ties go to the lowest variant,
    then to the first placement in row-major order.  With return_maps also maps: per variant the dict placement_scores returns for the transformed
    object (its arrays are views of one buffer; the same bits), None for a skipped variant.  Deterministic; a pair's numbers do not depend on the
    other pairs.  GPU only: CPU tensors raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    fn = "placement_search"
    s_b, ups_b, lats_b = _field_list("background", up_bg, lat_bg, fn)
    s_o, ups_o, lats_o = _field_list("object", up_obj, lat_obj, fn)
    if not ups_b or not ups_o:
        raise ValueError(f"{fn} needs at least one background and one object")
    every = ups_b + lats_b + ups_o + lats_o
    if not all(torch.is_tensor(t) for t in every):
        raise TypeError(f"{fn} takes torch tensors")
    for u, l in zip(ups_b + ups_o, lats_b + lats_o):
        if u.dim() != 3 or u.shape[0] != 2 or min(u.shape[1:]) < 1 or tuple(l.shape) != tuple(u.shape[1:]):
            raise ValueError(f"up must be (2, H, W) and lat (H, W) with H, W >= 1; got {tuple(u.shape)} and {tuple(l.shape)}")
    sc = _variant_values("scales", scales, fn)[1]
    ro = _variant_values("rotations", rotations, fn)[1]
    variants = [(s, r) for s in sc for r in ro]
    V = len(variants)
    stride = operator.index(stride)
    if stride < 1:
        raise ValueError(f"stride must be at least 1; got {stride}")
    min_valid = float(min_valid)
    if not 0.0 <= min_valid <= 1.0:
        raise ValueError(f"min_valid must be in [0, 1]; got {min_valid}")
    w_up, w_lat = (float(v) for v in weights)
    if not (w_up >= 0.0 and w_lat >= 0.0 and np.isfinite(w_up) and np.isfinite(w_lat)):
        raise ValueError(f"weights must be two finite numbers >= 0; got {weights}")
    nb, no = len(ups_b), len(ups_o)
    if pairs is None:
        plist = [(b, o) for b in range(nb) for o in range(no)]
    else:
        plist = [(operator.index(b), operator.index(o)) for b, o in (pairs.tolist() if torch.is_tensor(pairs) else pairs)]
        if not plist:
            raise ValueError(f"{fn} needs at least one pair")
    single = s_b and s_o and len(plist) == 1
    for b, o in plist:
        if not (0 <= b < nb and 0 <= o < no):
            raise ValueError(f"a pair is (background, object) with indices in [0, {nb}) and [0, {no}); got ({b}, {o})")
    masks = _masked_latitudes(lats_o, mask, "objects", fn)
    every += [m for m in masks if m is not None]
    if not all(t.is_cuda for t in every):
        raise PfError(f"{fn} runs on the GPU only (no CPU path)")
    dev = every[0].device
    if any(t.device != dev for t in every):
        raise ValueError(f"{fn}: all fields and masks must be on one device")
    ups_b, lats_b, ups_o, lats_o = ([t.to(torch.float32).contiguous() for t in ts] for ts in (ups_b, lats_b, ups_o, lats_o))
    lats_o = [l if m is None else torch.where(m, l, torch.full_like(l, float("nan"))) for l, m in zip(lats_o, masks)]
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    sizes = lambda ts: (ctypes.c_int32 * (2 * len(ts)))(*[s for u in ts for s in (int(u.shape[1]), int(u.shape[2]))])
    hw_b, hw_o = sizes(ups_b), sizes(ups_o)
    n_pair = len(plist)
    c_pairs = (ctypes.c_int32 * (2 * n_pair))(*[i for bo in plist for i in bo])
    c_var = (ctypes.c_double * (2 * V))(*[x for sr in variants for x in sr])
    lib = load_library()
    need = int(lib.pf_place_search_workspace_bytes(nb, hw_b, no, hw_o, n_pair, c_pairs, V, c_var, stride))
    if need == 0:
        raise ValueError(f"{fn}: sizes that one call does not take (a field or a transformed object of 2^31 pixels or more, or of more than 65535 x 1024)")
    # the sizes of the maps, as the library lays them out: the transformed size of every (object, variant)
    ohw = {}
    for o in {o for _, o in plist}:
        for v, (s, r) in enumerate(variants):
            hw = (ctypes.c_int32 * 2)()
            _check(lib.pf_fields_transform_size(int(ups_o[o].shape[1]), int(ups_o[o].shape[2]), s, r, hw), None, "pf_fields_transform_size")
            ohw[o, v] = (hw[0], hw[1])
    dims = []   # per pair, per variant: (P, Q) or None
    for b, o in plist:
        H, W = ups_b[b].shape[1:]
        dims.append([((H - ohw[o, v][0]) // stride + 1, (W - ohw[o, v][1]) // stride + 1) if ohw[o, v][0] <= H and ohw[o, v][1] <= W else None for v in range(V)])
    n_maps = 3 * sum(d[0] * d[1] for dv in dims for d in dv if d is not None)
    maps = torch.empty(max(n_maps, 1), dtype=torch.float64, device=dev)
    best = torch.empty((n_pair, 7), dtype=torch.float64, device=dev)
    var = torch.empty((n_pair, V, 6), dtype=torch.float64, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib.pf_place_search(dev.index, nb, ptrs(ups_b), ptrs(lats_b), hw_b, no, ptrs(ups_o), ptrs(lats_o), hw_o, n_pair, c_pairs, V, c_var, stride,
                                   min_valid, w_up, w_lat, maps.data_ptr(), n_maps, best.data_ptr(), var.data_ptr(), ws.data_ptr(), need, _stream_ptr()),
               None, "pf_place_search")
    t_var = torch.tensor(variants + [(float("nan"), float("nan"))], dtype=torch.float64, device=dev)   # row -1: no variant
    t_size = var[..., 4:6].to(torch.int64)
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=dev)
    res, first = [], 0
    for k, dv in enumerate(dims):
        bv = best[k, 4].to(torch.int64)
        d = dict(best_scale=t_var[bv, 0], best_rotation_deg=t_var[bv, 1], best_variant=bv, best_offset=best[k, 5:7].to(torch.int64), best_pfd_deg=best[k, 0],
                 best_up_mean_deg=best[k, 1], best_lat_mean_deg=best[k, 2],
                 best_size=torch.where(bv >= 0, t_size[k][bv.clamp(min=0)], torch.full_like(t_size[k][0], -1)),
                 variant_pfd_deg=var[k, :, 0], variant_offset=var[k, :, 1:3].to(torch.int64), variant_size=t_size[k],
                 variant_valid_pixels=var[k, :, 3].to(torch.int64), stride=stride)
        if return_maps:
            ms = []
            for v, pq in enumerate(dv):
                if pq is None:
                    ms.append(None)
                    continue
                P, Q = pq
                rec = maps[first:first + 3 * P * Q].view(P, Q, 3)
                first += 3 * P * Q
                n = rec[..., 2]
                up_mean, lat_mean = rec[..., 0] / n, rec[..., 1] / n
                ok = (n >= min_valid * var[k, v, 3]) & (n > 0)
                at = var[k, v, 1:3].to(torch.int64)
                ms.append(dict(pfd_deg=torch.where(ok, w_up * up_mean + w_lat * lat_mean, inf), up_mean_deg=up_mean, lat_mean_deg=lat_mean,
                               valid_pixels=n.to(torch.int64), best_offset=at, best_pfd_deg=var[k, v, 0], stride=stride))
            d["maps"] = ms
        res.append(d)
    return res[0] if single else res


COMPOSITE_SOFT, COMPOSITE_HARD = 0, 1   # include/pf_hip.h PF_COMPOSITE_*
_EDGES = {"soft": COMPOSITE_SOFT, "hard": COMPOSITE_HARD}


def _placement_columns(fn, name, v, width, n):
    """a per-job parameter of composite_objects -> (is a tensor, `width` columns): host numbers give lists of n floats, a device tensor gives float64
    tensors of shape (n,) that were never read"""
    if torch.is_tensor(v):
        shape = tuple(v.shape)
        ok = shape in ((), (n,)) if width == 1 else shape in ((width,), (n, width))
        if not ok or v.dtype == torch.bool or v.is_complex():
            raise ValueError(f"{fn}: {name} as a tensor is {'a number or (n,)' if width == 1 else f'({width},) or (n, {width})'} for n = {n} jobs; got {shape}")
        t = v.to(torch.float64).reshape(-1, width).expand(n, width)
        return True, [t[:, i] for i in range(width)]
    try:
        a = np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: {name} must be numbers or a tensor; got {v!r}") from None
    ok = a.shape in ((), (n,)) if width == 1 else a.shape in ((width,), (n, width))
    if not ok:
        raise ValueError(f"{fn}: {name} is {'a number or n numbers' if width == 1 else f'{width} numbers or n rows of them'} for n = {n} jobs; got shape {a.shape}")
    a = np.broadcast_to(a.reshape(-1, width), (n, width))
    return False, [[float(x) for x in a[:, i]] for i in range(width)]


def composite_objects(backgrounds, objects, *, scale=1.0, rotation=0.0, offset, size=None, alpha=None, pairs=None, opacity=1.0, edge="soft", samples=1,
                      return_coverage=False):
    """Objects pasted into background pictures on the GPU: the object's pixels resized by `scale` and turned by `rotation` degrees about its centre
    (transform_fields' similarity, so the pixels move as the fields did), alpha-blended into the background at `offset`.  It consumes what
    placement_search finds -- its best_scale, best_rotation_deg, best_offset and best_size can be passed as the device tensors they are, and nothing is
    read back.  Definitions: include/pf_hip.h pf_composite.

    backgrounds, objects: a CUDA tensor (H, W, 3), a batch (B, H, W, 3), or a list of (H, W, 3) tensors whose sizes may differ; uint8 or float32 on the
    0 - 255 scale, one dtype and one device for all.  An object may have 4 channels: colour and alpha on the 0 - 255 scale.  alpha: a bool or float
    (h, w) tensor in [0, 1] (one, or a list with one entry per object, None entries allowed), None = opaque; NaN counts as 0.
    pairs: (background, object) indices, one job each; default every background with every object, backgrounds outermost (placement_search's order).
    Per job, as host numbers (one for all jobs or one per job) or as device tensors (0-d / (n,), offset and size (2,) / (n, 2)):
    scale > 0; rotation in degrees, positive = clockwise on the screen; offset = (row, col) of the top-left corner of the transformed object's box in
    the background, which may be negative or hang over the border (the paste is clipped); size = (h', w') of that box, default the size
    transform_fields gives, which needs scale and rotation as host numbers: with tensors pass size=.  A job whose values cannot be pasted -- a scale
    that is not finite and > 0, a non-finite rotation, an offset that is not integer-valued, a size below 1 (placement_search's "nothing fits") --
    returns its background unchanged.
    opacity in [0, 1] multiplies the alpha.  edge="soft": the premultiplied bilinear mix, the object's outline and the array border fade over a pixel;
    edge="hard": a pixel is pasted in full where the resampled alpha is at least 1/2 and not at all elsewhere -- transform_fields' silhouette, the
    pixels the search scored.  samples=S in 1 .. 4: every pixel is the mean of S x S sub-samples (antialiasing for scale < 1), as for the gathers.
    Returns the composites: (H, W, 3) for one background tensor and one object tensor, (n, H, W, 3) for one background or a batch of them, a list for
    a list; with return_coverage also the coverage in [0, 1], float32, (H, W) per job in the same arrangement.  A pixel that is not covered keeps
    the background's bits.  uint8 results are rounded half up.  One C call on the current stream, no host synchronisation.  Deterministic; a
    job's bits do not depend on the other jobs.  GPU only: CPU tensors raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    fn = "composite_objects"
    kind_b, bgs = _draw_images(fn, backgrounds)
    kind_o, objs = _draw_images(fn, objects)
    if not all(torch.is_tensor(t) for t in bgs + objs):
        raise TypeError(f"{fn} takes torch tensors")
    for what, kind, ts, chans in (("a background", kind_b, bgs, (3,)), ("an object", kind_o, objs, (3, 4))):
        for t in ts:
            if t.dim() != (4 if kind == "batched" else 3) or t.shape[-1] not in chans or min(t.shape[-3:-1]) < 1 or (kind == "batched" and t.shape[0] < 1):
                raise ValueError(f"{fn}: {what} must be (H, W, {' or '.join(map(str, chans))}) with H, W >= 1, or a non-empty batch of them; got {tuple(t.shape)}")
            if t.dtype not in _PANO_DTYPES:
                raise ValueError(f"{fn}: images must be uint8 or float32; got {t.dtype}")
    if not bgs or not objs:
        raise ValueError(f"{fn} needs at least one background and one object")
    if len({t.dtype for t in bgs + objs}) != 1:
        raise ValueError(f"{fn}: backgrounds and objects must have one dtype")
    bgs = list(bgs[0].unbind(0)) if kind_b == "batched" else bgs
    objs = list(objs[0].unbind(0)) if kind_o == "batched" else objs
    if len({o.shape[-1] for o in objs}) != 1:
        raise ValueError(f"{fn}: the objects must all have 3 or all have 4 channels")
    nb, no = len(bgs), len(objs)
    if objs[0].shape[-1] == 4:
        if alpha is not None:
            raise ValueError(f"{fn}: alpha= with 4-channel objects, which carry their own")
        alphas = [o[..., 3].to(torch.float32) / 255.0 for o in objs]
        objs = [o[..., :3] for o in objs]
    else:
        alphas = [None] * no if alpha is None else [alpha] if torch.is_tensor(alpha) else list(alpha)
        if len(alphas) != no:
            raise ValueError(f"{fn}: {len(alphas)} alpha planes for {no} objects")
        for a, o in zip(alphas, objs):
            if a is not None and (not torch.is_tensor(a) or tuple(a.shape) != tuple(o.shape[:2]) or not (a.dtype == torch.bool or a.is_floating_point())):
                raise ValueError(f"{fn}: an alpha is a bool or float tensor of its object's size {tuple(o.shape[:2])}")
    if pairs is None:
        plist = [(b, o) for b in range(nb) for o in range(no)]
    else:
        plist = [(operator.index(b), operator.index(o)) for b, o in (pairs.tolist() if torch.is_tensor(pairs) else pairs)]
        if not plist:
            raise ValueError(f"{fn} needs at least one pair")
    for b, o in plist:
        if not (0 <= b < nb and 0 <= o < no):
            raise ValueError(f"a pair is (background, object) with indices in [0, {nb}) and [0, {no}); got ({b}, {o})")
    n = len(plist)
    opacity = float(opacity)
    if not 0.0 <= opacity <= 1.0:
        raise ValueError(f"opacity must be in [0, 1]; got {opacity}")
    if edge not in _EDGES:
        raise ValueError(f"edge must be 'soft' or 'hard'; got {edge!r}")
    samples = _check_samples(fn, samples)
    t_scale, (c_scale,) = _placement_columns(fn, "scale", scale, 1, n)
    t_rot, (c_rot,) = _placement_columns(fn, "rotation", rotation, 1, n)
    t_off, c_off = _placement_columns(fn, "offset", offset, 2, n)
    if size is None:
        if t_scale or t_rot:
            raise ValueError(f"{fn}: scale or rotation as tensors are not read back, so the size of the transformed object cannot be derived: pass size=")
        if not all(np.isfinite(s) and s > 0.0 for s in c_scale) or not all(np.isfinite(r) for r in c_rot):
            raise ValueError(f"{fn}: without size=, scale must be finite and > 0 and rotation finite; got {c_scale}, {c_rot}")
        t_size, c_size = False, None
    else:
        t_size, c_size = _placement_columns(fn, "size", size, 2, n)
    params = [c for is_t, cs in ((t_scale, [c_scale]), (t_rot, [c_rot]), (t_off, c_off), (t_size, c_size or [])) if is_t for c in cs]
    every = bgs + objs + [a for a in alphas if a is not None] + params
    if not all(t.is_cuda for t in every):
        raise PfError(f"{fn} runs on the GPU only (no CPU path)")
    dev = bgs[0].device if bgs[0].device.index is not None else torch.device("cuda", torch.cuda.current_device())
    if any((t.device if t.device.index is not None else torch.device("cuda", torch.cuda.current_device())) != dev for t in every):
        raise ValueError(f"{fn}: images, alphas and placement tensors must be on one device")
    lib = load_library()
    if c_size is None:
        c_size = [[], []]
        for (b, o), s, r in zip(plist, c_scale, c_rot):
            hw = (ctypes.c_int32 * 2)()
            if lib.pf_fields_transform_size(int(objs[o].shape[0]), int(objs[o].shape[1]), s, r, hw) != 0:
                raise ValueError(f"{fn}: {lib.pf_last_error(None).decode()}")
            c_size[0].append(float(hw[0]))
            c_size[1].append(float(hw[1]))
    cols = [c_scale, c_rot, *c_off, *c_size]
    if any(torch.is_tensor(c) for c in cols):
        place = torch.stack([c if torch.is_tensor(c) else torch.tensor(c, dtype=torch.float64, device=dev) for c in cols], 1).contiguous()
    else:
        place = torch.tensor([list(row) for row in zip(*cols)], dtype=torch.float64, device=dev)
    bgs, objs = [t.contiguous() for t in bgs], [t.contiguous() for t in objs]
    alphas = [None if a is None else a.to(torch.float32).contiguous() for a in alphas]
    same = len({tuple(bgs[b].shape) for b, _ in plist}) == 1
    if kind_b != "list" and same:
        stack = torch.empty((n,) + tuple(bgs[0].shape), dtype=bgs[0].dtype, device=dev)
        outs = list(stack.unbind(0))
    else:
        stack, outs = None, [torch.empty_like(bgs[b]) for b, _ in plist]
    npx = [int(bgs[b].shape[0]) * int(bgs[b].shape[1]) for b, _ in plist]
    cov = torch.empty(sum(npx), dtype=torch.float32, device=dev) if return_coverage else None
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    sizes = lambda ts: (ctypes.c_int32 * (2 * len(ts)))(*[int(s) for t in ts for s in t.shape[:2]])
    c_jobs = (ctypes.c_int32 * (2 * n))(*[i for bo in plist for i in bo])
    need = int(lib.pf_composite_workspace_bytes(n))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib.pf_composite(dev.index, nb, ptrs(bgs), sizes(bgs), no, ptrs(objs), ptrs(alphas), sizes(objs), _PANO_DTYPES[bgs[0].dtype], n, c_jobs,
                                place.data_ptr(), opacity, _EDGES[edge], samples, ptrs(outs), None if cov is None else cov.data_ptr(), ws.data_ptr(), need,
                                _stream_ptr()), None, "pf_composite")
    single = kind_b == "single" and kind_o == "single" and n == 1
    res = outs[0] if single else outs if stack is None else stack
    if not return_coverage:
        return res
    first = np.concatenate([[0], np.cumsum(npx)])
    covs = [cov[first[k]:first[k + 1]].view(bgs[b].shape[0], bgs[b].shape[1]) for k, (b, _) in enumerate(plist)]
    return res, (covs[0] if single else covs if stack is None else cov.view(n, *bgs[0].shape[:2]))


class FieldErrorAccumulator:
    """Dataset-level statistics of the field errors: a histogram of 1/64 degree bins over [0, 180] per metric (errors beyond land in
    the last bin) plus exact running totals, kept on `device`.  The state is additive, so it merges across batches (update /
    add_errors), accumulators (merge) and ranks (all_reduce).  summary() gives mean, rmse, max and frac_below exactly (fp64 sums,
    integer counts) and the MEDIAN TO WITHIN ONE BIN (1/64 degree): the centres of the bins that hold the two middle ranks."""

    def __init__(self, device, threshold_deg=5.0):
        self.device = torch.device(device)
        self.threshold_deg = float(threshold_deg)
        if not (self.threshold_deg > 0.0 and np.isfinite(self.threshold_deg)):
            raise ValueError("threshold_deg must be finite and > 0")
        self.hist = torch.zeros((2, _FERR_BINS), dtype=torch.int64, device=self.device)      # (up, lat) x bins
        self.sums = torch.zeros((2, len(_FERR_SUMS)), dtype=torch.float64, device=self.device)  # (up, lat) x (n, sum, sum_sq, max, below)

    def update(self, up_pred, lat_pred, up_gt, lat_gt, return_maps=False):
        """field_errors of one batch on the GPU, added to the state by the same call; returns its per-image dicts."""
        if self.device.type != "cuda":
            raise PfError("FieldErrorAccumulator.update runs on the GPU only; add_errors takes ready-made error maps on any device")
        return _field_errors(up_pred, lat_pred, up_gt, lat_gt, self.threshold_deg, return_maps, self.hist, self.sums)

    def add_errors(self, err_up, err_lat):
        """Adds ready-made error maps (tensors or lists of tensors, degrees, NaN = invalid, e.g. the maps field_errors returned) with
        torch ops on the accumulator's device: bookkeeping, the same bins as the kernel (min(int(e * 64), 11519) in fp32)."""
        for m, e in enumerate((err_up, err_lat)):
            for t in ([e] if torch.is_tensor(e) else list(e)):
                v = t.to(device=self.device, dtype=torch.float32).reshape(-1)
                v = v[~torch.isnan(v)]
                if v.numel() == 0:
                    continue
                bins = (v * float(_FERR_BINS_PER_DEG)).clamp(max=float(_FERR_BINS - 1)).to(torch.int64)
                self.hist[m] += torch.bincount(bins, minlength=_FERR_BINS)
                d = v.to(torch.float64)
                self.sums[m, 0] += v.numel()
                self.sums[m, 1] += d.sum()
                self.sums[m, 2] += (d * d).sum()
                self.sums[m, 3] = torch.maximum(self.sums[m, 3], d.max())
                self.sums[m, 4] += (v < self.threshold_deg).sum()
        return self

    def merge(self, other):
        if other.threshold_deg != self.threshold_deg:
            raise ValueError("merge needs accumulators of one threshold_deg")
        o_sums = other.sums.to(self.device)
        self.hist += other.hist.to(self.device)
        mx = torch.maximum(self.sums[:, 3], o_sums[:, 3])
        self.sums += o_sums
        self.sums[:, 3] = mx
        return self

    def all_reduce(self, group=None):
        """Combines the state over a torch.distributed group (sums; a max for the maxima), so every rank holds the statistics of the
        union -- composes with ShardedPerspectiveFields.  A no-op without an initialised process group."""
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized()):
            return self
        mx = self.sums[:, 3].clone()
        dist.all_reduce(self.hist, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.sums, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(mx, op=dist.ReduceOp.MAX, group=group)
        self.sums[:, 3] = mx
        return self

    def summary(self):
        """{up_mean_deg, up_median_deg, up_rmse_deg, up_max_deg, up_frac_below, lat_*..., valid_pixels} as Python numbers (reads the
        state back: synchronises).  The median is accurate to one bin, 1/64 degree; everything else is exact.  No pixel: NaN."""
        hist, sums = self.hist.cpu().numpy(), self.sums.cpu().numpy()
        out = {}
        for m, name in enumerate(("up", "lat")):
            n, s, s2, mx, below = (float(x) for x in sums[m])
            if n == 0:
                vals = [float("nan")] * 5
            else:
                cum = np.cumsum(hist[m])
                mid = [int(np.searchsorted(cum, r, side="right")) for r in ((int(n) - 1) // 2, int(n) // 2)]
                med = 0.5 * sum((b + 0.5) / _FERR_BINS_PER_DEG for b in mid)
                vals = [s / n, med, float(np.sqrt(s2 / n)), mx, below / n]
            for k, v in zip(_FERR_COLS[5 * m:5 * m + 5], vals):
                out[k] = v
        out["valid_pixels"] = int(sums[0, 0])
        return out


# panorama element types of pf_pano_crop (include/pf_hip.h PF_PANO_*)
PANO_U8, PANO_F32 = 0, 1
_PANO_DTYPES = {torch.uint8: PANO_U8, torch.float32: PANO_F32}


def _cuda_image_list(fn, items, nouns, spec, min_side, ndim=3):
    """the sources of a gather: a non-empty list of (H, W, 3) CUDA tensors (ndim=4: the one tensor (B, H, W, 3)) of one dtype and one device with
    H, W >= min_side -> (list, device with its index).  nouns = (a source, sources); spec: the shape as the message words it"""
    if not items:
        raise ValueError(f"{fn} needs at least one {nouns[0]}")
    if not all(torch.is_tensor(p) for p in items):
        raise TypeError(f"{fn} takes torch tensors as {nouns[1]}")
    if not all(p.is_cuda for p in items):
        raise PfError(f"{fn} runs on the GPU only (no CPU path)")
    for p in items:
        if p.dim() != ndim or p.shape[-1] != 3 or p.shape[-2] < min_side or p.shape[-3] < min_side:
            raise ValueError(f"{spec}; got {tuple(p.shape)}")
        if p.dtype not in _PANO_DTYPES:
            raise ValueError(f"{nouns[1]} must be uint8 or float32; got {p.dtype}")
    if len({p.dtype for p in items}) != 1 or len({p.device for p in items}) != 1:
        raise ValueError(f"{fn}: all {nouns[1]} must have one dtype and one device")
    dev = items[0].device
    return items, dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def _broadcast_len(fn, ts):
    """the batch size that checked parameter tensors (numbers or 1-d) broadcast to, 1 when all are scalars; nothing moves to the device"""
    try:
        shape = torch.broadcast_shapes(*[tuple(t.shape) for t in ts])
    except RuntimeError as e:
        raise ValueError(f"{fn}: camera parameters do not broadcast: {e}") from None
    return int(shape[0]) if shape else 1


def _camera_rows(ts, angles, B, dev, mode):
    """parameter tensors that broadcast to B -> (B, len(ts)) fp32 rows on the device, after every check of the caller.  As fields_from_params:
    the `angles` columns go from degrees to radians in fp64 (mode "deg"), then everything to fp32"""
    ts = [t.to(device=dev, dtype=torch.float64) for t in ts]
    if mode == "deg":
        for k in angles:
            ts[k] = torch.deg2rad(ts[k])
    return torch.stack([t.expand(B) for t in ts], 1).to(torch.float32)


GATHER_MAX_SAMPLES = 4   # include/pf_hip.h PF_GATHER_MAX_SAMPLES


def _check_samples(fn, samples):
    """`samples` of a gather: an int in 1 .. GATHER_MAX_SAMPLES (the side of the grid of sub-samples per output pixel)"""
    if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or not 1 <= samples <= GATHER_MAX_SAMPLES:
        raise ValueError(f"{fn}: samples must be an integer in [1, {GATHER_MAX_SAMPLES}]; got {samples!r}")
    return int(samples)


def _source_arrays(srcs, sizes, idx):
    """the ctypes arguments that name a gather's sources: their pointers, their (H, W) pairs, the source of each output"""
    n = len(srcs)
    return ((ctypes.c_void_p * n)(*[p.data_ptr() for p in srcs]), (ctypes.c_int32 * (2 * n))(*[s for hw in sizes for s in hw]),
            (ctypes.c_int32 * len(idx))(*idx))


def crop_panorama(pano, roll, pitch, rel_focal, rel_cx=0.0, rel_cy=0.0, *, yaw=0.0, xi=0.0, height, width, pano_index=None, mode="deg", fields=True, samples=1):
    """Equirectangular panoramas -> camera views and their ground-truth perspective fields on the GPU: the reference's labelled-data
    tooling (PanoCam.get_image / crop_equi, crop_distortion for the Unified Spherical Model, get_up_general / get_lat_general in
    utils/panocam.py).  Camera model, sampling and labels: include/pf_hip.h pf_pano_crop.

    pano: a CUDA tensor (Hp, Wp, 3), uint8 or float32, or a list of them (one dtype, one device).
    roll, pitch, yaw (degrees unless mode="rad"), rel_focal, rel_cx, rel_cy, xi (0: pinhole; > 0: Unified Spherical Model): numbers,
    0-d tensors or 1-d tensors / sequences, broadcast to the batch size B (1 when all are scalars); device tensors stay on the device.
    pano_index: None (every crop from panorama 0) or B integers.  height, width: the size of every crop.
    Returns (images (B, H, W, 3) in the panorama's dtype, up (B, 2, H, W), lat (B, H, W) degrees); up / lat are None with fields=False.
    The labels use the layout of pred_gravity_original / pred_latitude_original; at xi = 0 they are bit-identical to
    `fields_from_params` with the same arguments.  Pixels without a ray (xi > 1) are 0 in the image and NaN in the labels.

    The orientation conventions are those of `fields_from_params` (pinned to the reference by tests/golden): x right, y down,
    positive pitch looks up, positive yaw turns towards higher panorama columns, row 0 of the panorama is the north pole and its
    centre column is longitude 0.  samples=S (1 .. 4) antialiases a crop that minifies its panorama: every pixel is the mean of S x S bilinear
    sub-samples (include/pf_hip.h pf_pano_crop_ss); the labels do not depend on it, and S = 1 is the one sample at the pixel centre.
    Pixel parity with the reference's equilib backend is not checked.  The reference's
    get_image(vfov, im_w, im_h, azimuth, elevation, roll, ar) maps to height=im_h, width=im_w, yaw=azimuth, pitch=elevation, roll=roll,
    rel_focal = 0.5 / tan(vfov / 2) (a centred crop with square pixels), rel_cx = rel_cy = 0, xi = 0.
    GPU only: CPU panoramas raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    samples = _check_samples("crop_panorama", samples)
    panos, dev = _cuda_image_list("crop_panorama", [pano] if torch.is_tensor(pano) else list(pano), ("panorama", "panoramas"),
                                  "a panorama must be (Hp, Wp, 3) with Hp, Wp >= 2", 2)
    H, W = int(height), int(width)
    if H < 1 or W < 1:
        raise ValueError(f"crop size must be at least 1 x 1; got {H} x {W}")
    if mode not in ("deg", "rad"):
        raise ValueError("mode must be 'deg' or 'rad'")
    ts = []   # validated where they are; moved to the device after every check
    for name, v in (("roll", roll), ("pitch", pitch), ("yaw", yaw), ("rel_focal", rel_focal), ("rel_cx", rel_cx), ("rel_cy", rel_cy), ("xi", xi)):
        t = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.float64))
        if t.dim() > 1:
            raise ValueError(f"{name} must be a number or a 1-d sequence; got shape {tuple(t.shape)}")
        ts.append(t)
    B = _broadcast_len("crop_panorama", ts)
    if B < 1:
        raise ValueError("crop_panorama needs at least one crop")
    if pano_index is None:
        idx = [0] * B
    else:
        idx = [operator.index(i) for i in (pano_index.tolist() if torch.is_tensor(pano_index) else pano_index)]
        if len(idx) != B:
            raise ValueError(f"pano_index has {len(idx)} entries for {B} crops")
        if any(i < 0 or i >= len(panos) for i in idx):
            raise ValueError(f"pano_index entries must be in [0, {len(panos)})")
    cam = _camera_rows(ts, (0, 1, 2), B, dev, mode).contiguous()
    panos = [p.contiguous() for p in panos]
    img = torch.empty((B, H, W, 3), dtype=panos[0].dtype, device=dev)
    up = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev) if fields else None
    lat = torch.empty((B, H, W), dtype=torch.float32, device=dev) if fields else None
    p_pano, hw, c_idx = _source_arrays(panos, [(int(p.shape[0]), int(p.shape[1])) for p in panos], idx)
    lib = load_library()
    with torch.cuda.device(dev):
        args = (dev.index, len(panos), p_pano, hw, _PANO_DTYPES[panos[0].dtype], B, c_idx, cam.data_ptr(), H, W, img.data_ptr(),
                up.data_ptr() if fields else None, lat.data_ptr() if fields else None)
        if samples == 1:
            _check(lib.pf_pano_crop(*args, _stream_ptr()), None, "pf_pano_crop")
        else:
            _check(lib.pf_pano_crop_ss(*args, samples, _stream_ptr()), None, "pf_pano_crop_ss")
    return img, up, lat


def _rotation_params(fn, named):
    """(name, value) pairs -> tensors (numbers or 1-d), checked where they are; nothing moves to the device"""
    ts = []
    for name, v in named:
        t = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.float64))
        if t.dim() > 1:
            raise ValueError(f"{fn}: {name} must be a number or a 1-d sequence; got shape {tuple(t.shape)}")
        ts.append(t)
    return ts


def rotate_panorama(pano, roll=0.0, pitch=0.0, yaw=0.0, *, inverse=False, height=None, width=None, pano_index=None, mode="deg", fields=False, samples=1):
    """Equirectangular panoramas -> rotated equirectangular panoramas on the GPU, with the perspective fields of the panoramic camera on request:
    levelling a tilted 360 degree picture, tilting an upright one (labelled data for tilted panoramas), re-centring a composite.  Model, sampling and
    labels: include/pf_hip.h pf_pano_rotate; the conventions are `crop_panorama`'s.

    pano: a CUDA tensor (Hs, Ws, 3), uint8 or float32, or a list of them (one dtype, one device).
    roll, pitch, yaw (degrees unless mode="rad"): numbers, 0-d tensors or 1-d tensors / sequences, broadcast to the batch size B (1 when all are
    scalars); device tensors stay on the device.  With Q = Y(yaw) R_pitch(pitch) R_roll(roll):
    inverse=False -- the output is what a panoramic camera with orientation (roll, pitch, yaw) inside the (upright) source sees;
    inverse=True  -- a source shot by such a camera becomes the upright panorama: the levelling direction, which undoes the other.
    pano_index: None (every output from panorama 0) or B integers.  height, width: the size of every output, default the sources' (required
    when they differ in size).
    Returns the images (B, H, W, 3) in the panorama's dtype; with fields=True (images, up (B, 2, H, W), lat (B, H, W) degrees), the perspective
    fields of the output's camera in the layout of pred_gravity_original / pred_latitude_original (up is NaN at a pixel centre on the world's zenith
    or nadir).  Non-finite angles give an image of 0 and NaN fields.  samples=S (1 .. 4) antialiases an output smaller than its source: every pixel
    is the mean of S x S bilinear sub-samples (include/pf_hip.h pf_pano_rotate_ss); the fields do not depend on it.
    GPU only: CPU panoramas raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    samples = _check_samples("rotate_panorama", samples)

    panos, dev = _cuda_image_list("rotate_panorama", [pano] if torch.is_tensor(pano) else list(pano), ("panorama", "panoramas"),
                                  "a panorama must be (Hs, Ws, 3) with Hs, Ws >= 2", 2)
    sizes = [(int(p.shape[0]), int(p.shape[1])) for p in panos]
    if (height is None) != (width is None):
        raise ValueError("rotate_panorama: height and width are both given or both left out")
    if height is None:
        if len(set(sizes)) != 1:
            raise ValueError("rotate_panorama: the panoramas differ in size, so height and width are required")
        H, W = sizes[0]
    else:
        H, W = int(height), int(width)
    if H < 1 or W < 1:
        raise ValueError(f"output size must be at least 1 x 1; got {H} x {W}")
    if mode not in ("deg", "rad"):
        raise ValueError("mode must be 'deg' or 'rad'")
    ts = _rotation_params("rotate_panorama", (("roll", roll), ("pitch", pitch), ("yaw", yaw)))
    B = _broadcast_len("rotate_panorama", ts)
    if B < 1:
        raise ValueError("rotate_panorama needs at least one output")
    if pano_index is None:
        idx = [0] * B
    else:
        idx = [operator.index(i) for i in (pano_index.tolist() if torch.is_tensor(pano_index) else pano_index)]
        if len(idx) != B:
            raise ValueError(f"pano_index has {len(idx)} entries for {B} outputs")
        if any(i < 0 or i >= len(panos) for i in idx):
            raise ValueError(f"pano_index entries must be in [0, {len(panos)})")
    rot = _camera_rows(ts, (0, 1, 2), B, dev, mode).contiguous()
    panos = [p.contiguous() for p in panos]
    img = torch.empty((B, H, W, 3), dtype=panos[0].dtype, device=dev)
    up = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev) if fields else None
    lat = torch.empty((B, H, W), dtype=torch.float32, device=dev) if fields else None
    p_pano, hw, c_idx = _source_arrays(panos, sizes, idx)
    lib = load_library()
    with torch.cuda.device(dev):
        args = (dev.index, len(panos), p_pano, hw, _PANO_DTYPES[panos[0].dtype], B, c_idx, rot.data_ptr(), 1 if inverse else 0, H, W,
                img.data_ptr(), up.data_ptr() if fields else None, lat.data_ptr() if fields else None)
        if samples == 1:
            _check(lib.pf_pano_rotate(*args, _stream_ptr()), None, "pf_pano_rotate")
        else:
            _check(lib.pf_pano_rotate_ss(*args, samples, _stream_ptr()), None, "pf_pano_rotate_ss")
    return (img, up, lat) if fields else img


def panorama_fields(roll, pitch, *, height, width, mode="deg", device=None):
    """The perspective fields of an equirectangular (panoramic) camera with the given roll and pitch on the GPU: the counterpart of
    `fields_from_params` for the equirectangular projection, and the labels of `rotate_panorama(..., fields=True)` for the same parameters, bit for
    bit (yaw does not enter).  Model: include/pf_hip.h pf_pano_fields.
    roll, pitch (degrees unless mode="rad"): numbers, 0-d tensors or 1-d tensors / sequences, broadcast to B.  Returns (up (B, 2, H, W) unit vectors,
    latitude (B, H, W) degrees); up is NaN at a pixel centre on the zenith or nadir.  device: a CUDA device, default that of a tensor argument,
    else the current one."""
    from .engine import _check, _stream_ptr, load_library

    H, W = int(height), int(width)
    if H < 1 or W < 1:
        raise ValueError(f"field size must be at least 1 x 1; got {H} x {W}")
    if mode not in ("deg", "rad"):
        raise ValueError("mode must be 'deg' or 'rad'")
    ts = _rotation_params("panorama_fields", (("roll", roll), ("pitch", pitch), ("yaw", 0.0)))
    B = _broadcast_len("panorama_fields", ts)
    if B < 1:
        raise ValueError("panorama_fields needs at least one camera")
    if device is None:
        device = next((t.device for t in ts if t.is_cuda), None)
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise PfError("panorama_fields runs on the GPU only (no CPU path)")
    if not torch.cuda.is_available():
        raise PfError("panorama_fields runs on the GPU only and no GPU is available")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    rot = _camera_rows(ts, (0, 1, 2), B, dev, mode).contiguous()
    up = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
    lat = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    lib = load_library()
    with torch.cuda.device(dev):
        _check(lib.pf_pano_fields(dev.index, B, rot.data_ptr(), 0, H, W, up.data_ptr(), lat.data_ptr(), _stream_ptr()), None, "pf_pano_fields")
    return up, lat


_CUBE_FACES = ("front", "right", "back", "left", "up", "down")
_CUBE_PITCH_YAW = ((0.0, 0.0), (0.0, 90.0), (0.0, 180.0), (0.0, 270.0), (90.0, 0.0), (-90.0, 0.0))   # include/pf_hip.h, the cube-map convention
_CUBE_CROSS = ((1, 1), (1, 2), (1, 3), (1, 0), (0, 1), (2, 1))   # (block row, block column) of face k in the "cross" layout


def cubemap_face_cameras(mode="deg"):
    """The six cameras whose pictures are the faces front, right, back, left, up, down of a cube map (include/pf_hip.h, the cube-map convention):
    a dict of per-face lists roll, pitch, yaw (degrees, radians with mode="rad") and rel_focal = 0.5, the parameters `crop_panorama` and
    `compose_panorama` take: compose_panorama(faces, cubemap_face_cameras(), ...) turns six faces into a panorama by blending views,
    crop_panorama(pano, **cubemap_face_cameras(), height=N, width=N) cuts them."""
    if mode not in ("deg", "rad"):
        raise ValueError("mode must be 'deg' or 'rad'")
    conv = (lambda a: a) if mode == "deg" else (lambda a: float(np.radians(a)))
    return dict(roll=[0.0] * 6, pitch=[conv(p) for p, _ in _CUBE_PITCH_YAW], yaw=[conv(y) for _, y in _CUBE_PITCH_YAW], rel_focal=[0.5] * 6)


def _cube_list(fn, cube):
    """the cube maps of a gather: (6, N, N, 3) CUDA tensors of one dtype and one device -> (list, device)"""
    cubes, dev = _cuda_image_list(fn, [cube] if torch.is_tensor(cube) else list(cube), ("cube map", "cube maps"),
                                  "a cube map must be (6, N, N, 3) with N >= 1", 1, ndim=4)
    for c in cubes:
        if c.shape[0] != 6 or c.shape[1] != c.shape[2]:
            raise ValueError(f"a cube map must be (6, N, N, 3) with N >= 1; got {tuple(c.shape)}")
    return cubes, dev


def _cube_index(cube_index, B, n, what):
    if cube_index is None:
        return [0] * B
    idx = [operator.index(i) for i in (cube_index.tolist() if torch.is_tensor(cube_index) else cube_index)]
    if len(idx) != B:
        raise ValueError(f"cube_index has {len(idx)} entries for {B} {what}")
    if any(i < 0 or i >= n for i in idx):
        raise ValueError(f"cube_index entries must be in [0, {n})")
    return idx


def crop_cubemap(cube, roll, pitch, rel_focal, rel_cx=0.0, rel_cy=0.0, *, yaw=0.0, xi=0.0, height, width, cube_index=None, mode="deg", fields=True, samples=1):
    """Cube maps -> camera views and their ground-truth perspective fields on the GPU: `crop_panorama` for 360 degree material stored as six faces
    (skyboxes, environment maps, six-face camera exports), without a detour through a panorama.  Convention and sampling: include/pf_hip.h
    pf_cube_crop.

    cube: a CUDA tensor (6, N, N, 3), uint8 or float32, faces front, right, back, left, up, down (`cubemap_face_cameras`), or a list of them (one
    dtype, one device; N may differ).  The camera parameters, mode, height, width and samples are `crop_panorama`'s; cube_index: None (every view
    from cube 0) or B integers.  The bilinear sampler is continuous across the edges and corners of the cube: a view that straddles an edge has no
    seam.  Returns (images (B, H, W, 3) in the cube's dtype, up (B, 2, H, W), lat (B, H, W) degrees); up / lat are `fields_from_params` of the same
    parameters (they do not depend on the source) and None with fields=False.  Pixels without a ray (xi > 1) are 0; a view with a non-finite
    parameter is 0.  GPU only: CPU cubes raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    fn = "crop_cubemap"
    samples = _check_samples(fn, samples)
    cubes, dev = _cube_list(fn, cube)
    H, W = int(height), int(width)
    if H < 1 or W < 1:
        raise ValueError(f"view size must be at least 1 x 1; got {H} x {W}")
    if mode not in ("deg", "rad"):
        raise ValueError("mode must be 'deg' or 'rad'")
    ts = _rotation_params(fn, (("roll", roll), ("pitch", pitch), ("yaw", yaw), ("rel_focal", rel_focal), ("rel_cx", rel_cx), ("rel_cy", rel_cy), ("xi", xi)))
    B = _broadcast_len(fn, ts)
    if B < 1:
        raise ValueError(f"{fn} needs at least one view")
    idx = _cube_index(cube_index, B, len(cubes), "views")
    cam = _camera_rows(ts, (0, 1, 2), B, dev, mode).contiguous()
    cubes = [c.contiguous() for c in cubes]
    img = torch.empty((B, H, W, 3), dtype=cubes[0].dtype, device=dev)
    p_cube, hw, c_idx = _source_arrays(cubes, [(int(c.shape[1]), int(c.shape[2])) for c in cubes], idx)
    lib = load_library()
    with torch.cuda.device(dev):
        _check(lib.pf_cube_crop(dev.index, len(cubes), p_cube, hw, _PANO_DTYPES[cubes[0].dtype], B, c_idx, cam.data_ptr(), H, W, img.data_ptr(), samples,
                                _stream_ptr()), None, "pf_cube_crop")
    if not fields:
        return img, None, None
    pinhole = not torch.is_tensor(xi) and np.ndim(xi) == 0 and float(xi) == 0.0   # fields_from_params' rule: the number 0 is the pinhole model
    rows = [t.expand(B) for t in ts]
    per_view = [fields_from_params(rows[0][i], rows[1][i], rows[3][i], rows[4][i], rows[5][i], height=H, width=W, mode=mode, device=dev,
                                   xi=0.0 if pinhole else rows[6][i]) for i in range(B)]
    return img, torch.stack([u for u, _ in per_view]), torch.stack([l for _, l in per_view])


def cubemap_to_panorama(cube, *, height, width, roll=0.0, pitch=0.0, yaw=0.0, inverse=False, cube_index=None, mode="deg", fields=False, samples=1):
    """Cube maps -> equirectangular panoramas on the GPU, turned on the way if angles are given: a tilted cube map is levelled into a panorama in one
    pass.  Convention and sampling: include/pf_hip.h pf_cube_to_pano.

    cube: as `crop_cubemap`.  roll, pitch, yaw, inverse, mode, samples: `rotate_panorama`'s, with the cube in the place of the source panorama
    (inverse=False: what a panoramic camera with that orientation inside the cube sees; inverse=True: a cube shot by such a rig becomes upright).
    height, width: the size of every output; cube_index: None (every output from cube 0) or B integers.
    Returns the images (B, H, W, 3) in the cube's dtype; with fields=True (images, up, lat), the fields being `panorama_fields(roll, pitch)` (those
    of the output's camera for inverse=False).  Non-finite angles give an image of 0.  GPU only: CPU cubes raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    fn = "cubemap_to_panorama"
    samples = _check_samples(fn, samples)
    cubes, dev = _cube_list(fn, cube)
    H, W = int(height), int(width)
    if H < 1 or W < 1:
        raise ValueError(f"output size must be at least 1 x 1; got {H} x {W}")
    if mode not in ("deg", "rad"):
        raise ValueError("mode must be 'deg' or 'rad'")
    ts = _rotation_params(fn, (("roll", roll), ("pitch", pitch), ("yaw", yaw)))
    B = _broadcast_len(fn, ts)
    if B < 1:
        raise ValueError(f"{fn} needs at least one output")
    idx = _cube_index(cube_index, B, len(cubes), "outputs")
    rot = _camera_rows(ts, (0, 1, 2), B, dev, mode).contiguous()
    cubes = [c.contiguous() for c in cubes]
    img = torch.empty((B, H, W, 3), dtype=cubes[0].dtype, device=dev)
    p_cube, hw, c_idx = _source_arrays(cubes, [(int(c.shape[1]), int(c.shape[2])) for c in cubes], idx)
    lib = load_library()
    with torch.cuda.device(dev):
        _check(lib.pf_cube_to_pano(dev.index, len(cubes), p_cube, hw, _PANO_DTYPES[cubes[0].dtype], B, c_idx, rot.data_ptr(), 1 if inverse else 0, H, W,
                                   img.data_ptr(), samples, _stream_ptr()), None, "pf_cube_to_pano")
    if not fields:
        return img
    up, lat = panorama_fields(ts[0].expand(B), ts[1].expand(B), height=H, width=W, mode=mode, device=dev)
    return img, up, lat


# projection kinds and lens layout of the fisheye gathers (include/pf_hip.h PF_FISHEYE_*)
FISHEYE_PROJECTIONS = {"equidistant": 0, "equisolid": 1, "stereographic": 2}
FISHEYE_MAX_LENSES, FISHEYE_LENS_FLOATS = 2, 12
_FISHEYE_RHO = {"equidistant": lambda t: t, "equisolid": lambda t: 2.0 * np.sin(0.5 * t), "stereographic": lambda t: 2.0 * np.tan(0.5 * t)}


def _fisheye_kind(fn, projection):
    if projection not in FISHEYE_PROJECTIONS:
        raise ValueError(f"{fn}: projection must be one of {sorted(FISHEYE_PROJECTIONS)}; got {projection!r}")
    return FISHEYE_PROJECTIONS[projection]


def fisheye_lens(fov, *, radius, center, projection="equidistant", k=(0.0, 0.0, 0.0, 0.0), roll=0.0, pitch=0.0, yaw=0.0, band=0.0, mode="deg"):
    """One lens row of the fisheye gathers (include/pf_hip.h, the lens model): 12 float64 values {roll, pitch, yaw (radians), F, Cx, Cy, theta_max,
    k1, k2, k3, k4, band}, from what a user knows about the lens.

    fov: the full field of view, in (0, 360] degrees; `radius`: the radius in pixels of the image circle, where the ray at fov / 2 lands;
    center = (Cx, Cy): the circle's centre in pixel-edge units of the frame (a texel centre is at integer + 1/2); projection: "equidistant"
    (rho = theta), "equisolid" (2 sin(theta / 2)) or "stereographic" (2 tan(theta / 2)); k = (k1, k2, k3, k4): the Kannala-Brandt polynomial
    theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8), OpenCV's fisheye model with the equidistant kind; roll, pitch, yaw: the
    lens -> world rotation Y(yaw) R(roll, pitch) in the conventions of `crop_panorama`; band: the feather width, the angle before fov / 2 over
    which the lens fades out.  fov, band and the angles are degrees unless mode="rad".  F = radius / rho(theta_d(fov / 2)).
    r(theta) = rho(theta_d(theta)) is evaluated in fp64 on [0, fov / 2]; a ValueError is raised if it is not strictly increasing: the polynomial is
    then not a lens."""
    fn = "fisheye_lens"
    if mode not in ("deg", "rad"):
        raise ValueError("mode must be 'deg' or 'rad'")
    _fisheye_kind(fn, projection)
    conv = np.radians if mode == "deg" else (lambda a: a)
    vals = [float(v) for v in (fov, radius, band, roll, pitch, yaw)]
    cx, cy = (float(c) for c in center)
    ks = [float(v) for v in k]
    if len(ks) != 4:
        raise ValueError(f"{fn}: k has 4 coefficients (k1, k2, k3, k4); got {len(ks)}")
    if not np.isfinite(vals + [cx, cy] + ks).all():
        raise ValueError(f"{fn}: every value must be finite")
    tmax, band_r = 0.5 * float(conv(vals[0])), float(conv(vals[2]))
    if not 0.0 < tmax <= np.pi:
        raise ValueError(f"{fn}: fov must be in (0, {'360] degrees' if mode == 'deg' else '2 pi] radians'}; got {fov!r}")
    if not vals[1] > 0.0:
        raise ValueError(f"{fn}: radius must be > 0; got {radius!r}")
    if band_r < 0.0:
        raise ValueError(f"{fn}: band must be >= 0; got {band!r}")
    t = np.linspace(0.0, tmax, 4097)
    t2 = t * t
    td = t * (1.0 + t2 * (ks[0] + t2 * (ks[1] + t2 * (ks[2] + t2 * ks[3]))))
    with np.errstate(all="ignore"):
        r = _FISHEYE_RHO[projection](td)
    if not (np.isfinite(r).all() and (np.diff(r) > 0.0).all()):
        raise ValueError(f"{fn}: r(theta) is not strictly increasing on [0, fov / 2]: projection {projection!r} with k = {tuple(ks)} is not a lens")
    return np.array([conv(vals[3]), conv(vals[4]), conv(vals[5]), vals[1] / r[-1], cx, cy, tmax, *ks, band_r], dtype=np.float64)


def dual_fisheye_lenses(height, width, fov, **kw):
    """The two lens rows (2, 12) of the usual side-by-side dual-fisheye frame (height, width) of a two-lens 360 degree camera: image circles centred
    at (width / 4, height / 2) and (3 width / 4, height / 2) with radius min(width / 4, height / 2), the second lens at yaw + 180 degrees, and
    band = fov - 180 degrees, the overlap of the two lenses, so that one lens fades out exactly where the other fades in.  fov and the keywords
    projection, k, roll, pitch, yaw, mode (and band, to override the default) are `fisheye_lens`'s."""
    fn = "dual_fisheye_lenses"
    H, W = float(height), float(width)
    if not (H >= 1 and W >= 2):
        raise ValueError(f"{fn}: the frame must be at least 1 x 2; got {height} x {width}")
    if "radius" in kw or "center" in kw:
        raise TypeError(f"{fn}: radius and center follow from the frame")
    mode = kw.get("mode", "deg")
    if mode not in ("deg", "rad"):
        raise ValueError("mode must be 'deg' or 'rad'")
    half = 180.0 if mode == "deg" else np.pi
    band = kw.pop("band", max(float(fov) - half, 0.0))
    yaw = float(kw.pop("yaw", 0.0))
    radius = min(W / 4.0, H / 2.0)
    return np.stack([fisheye_lens(fov, radius=radius, center=(W / 4.0, H / 2.0), yaw=yaw, band=band, **kw),
                     fisheye_lens(fov, radius=radius, center=(3.0 * W / 4.0, H / 2.0), yaw=yaw + half, band=band, **kw)])


def _fisheye_frames(fn, frames):
    """the frames of a fisheye gather: (Hs, Ws, 3) CUDA tensors of one dtype and one device -> (list, device)"""
    return _cuda_image_list(fn, [frames] if torch.is_tensor(frames) else list(frames), ("frame", "frames"), "a frame must be (Hs, Ws, 3) with Hs, Ws >= 1", 1)


def _fisheye_lens_table(fn, lenses, n_frame):
    """`lenses` -> (n_frame, 2, 12) float64.  Anything 1-d or 2-d is ONE entry shared by every frame: a row (12,), or 1 or 2 rows ((1, 12), (2, 12),
    also as a list of two rows, so two rows are always the two lenses of a frame, never one lens each for two frames).  Per frame: an array
    (n_frame, 1 or 2, 12), or a list of n_frame 2-d entries ((1, 12) for a frame with one lens).  A missing second lens is a row of zeros:
    theta_max = 0 switches it off"""
    def host(e):
        return e.detach().cpu().numpy() if torch.is_tensor(e) else e

    def entry(e):
        a = np.asarray(host(e), dtype=np.float64)
        if a.ndim == 1:
            a = a[None]
        if a.ndim != 2 or a.shape[1] != FISHEYE_LENS_FLOATS or not 1 <= a.shape[0] <= FISHEYE_MAX_LENSES:
            raise ValueError(f"{fn}: a frame's lenses are one row of {FISHEYE_LENS_FLOATS} values or {FISHEYE_MAX_LENSES} such rows; got shape {tuple(a.shape)}")
        return np.concatenate([a, np.zeros((FISHEYE_MAX_LENSES - a.shape[0], FISHEYE_LENS_FLOATS))])

    ndim = lambda e: e.dim() if torch.is_tensor(e) else np.ndim(e)
    if isinstance(lenses, (list, tuple)):
        per_frame = len(lenses) > 0 and all(ndim(e) == 2 for e in lenses)
    else:
        per_frame = ndim(lenses) == 3
    if not per_frame:
        return np.repeat(entry(lenses)[None], n_frame, axis=0)
    if len(lenses) != n_frame:
        raise ValueError(f"{fn}: lenses has {len(lenses)} entries for {n_frame} frames")
    return np.stack([entry(e) for e in lenses])


def _frame_index(frame_index, B, n, what):
    if frame_index is None:
        return [0] * B
    idx = [operator.index(i) for i in (frame_index.tolist() if torch.is_tensor(frame_index) else frame_index)]
    if len(idx) != B:
        raise ValueError(f"frame_index has {len(idx)} entries for {B} {what}")
    if any(i < 0 or i >= n for i in idx):
        raise ValueError(f"frame_index entries must be in [0, {n})")
    return idx


def crop_fisheye(frames, lenses, roll, pitch, rel_focal, rel_cx=0.0, rel_cy=0.0, *, yaw=0.0, xi=0.0, height, width, frame_index=None, projection="equidistant",
                 mode="deg", fields=True, samples=1, fill=0, return_mask=False):
    """Fisheye and dual-fisheye frames -> camera views and their ground-truth perspective fields on the GPU: `crop_panorama` for the raw frames of a
    fisheye lens or of a two-lens 360 degree camera, without stitching a panorama first; with xi = 0 the view is the undistorted picture.  Lens
    model and sampling: include/pf_hip.h pf_fisheye_crop.

    frames: a CUDA tensor (Hs, Ws, 3), uint8 or float32, or a list of them (one dtype, one device; sizes may differ).  lenses: a row of
    `fisheye_lens`, a pair of rows (`dual_fisheye_lenses`; two lenses are blended across their overlap), both shared by every frame, or one such
    entry per frame (a list of (1 or 2, 12) arrays, or an array (n_frames, 1 or 2, 12)); two plain rows are always the two lenses of one frame,
    so two frames with one lens each take two (1, 12) entries.  The rows hold radians and are read on the host.
    projection: the kind of every lens of the call.  The camera parameters, mode, height, width and samples are `crop_panorama`'s; frame_index:
    None (every view from frame 0) or B integers.  fill: the value of the pixels without a ray or without a covering lens.
    Returns (images (B, H, W, 3) in the frames' dtype, up (B, 2, H, W), lat (B, H, W) degrees), and the mask (B, H, W) bool as a fourth entry with
    return_mask=True; up / lat are `fields_from_params` of the same parameters (they do not depend on the source) and None with fields=False.  A
    view with a non-finite parameter is `fill`.  GPU only: CPU frames raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    fn = "crop_fisheye"
    samples = _check_samples(fn, samples)
    kind = _fisheye_kind(fn, projection)
    srcs, dev = _fisheye_frames(fn, frames)
    H, W = int(height), int(width)
    if H < 1 or W < 1:
        raise ValueError(f"view size must be at least 1 x 1; got {H} x {W}")
    if mode not in ("deg", "rad"):
        raise ValueError("mode must be 'deg' or 'rad'")
    fill = float(fill)
    ts = _rotation_params(fn, (("roll", roll), ("pitch", pitch), ("yaw", yaw), ("rel_focal", rel_focal), ("rel_cx", rel_cx), ("rel_cy", rel_cy), ("xi", xi)))
    B = _broadcast_len(fn, ts)
    if B < 1:
        raise ValueError(f"{fn} needs at least one view")
    idx = _frame_index(frame_index, B, len(srcs), "views")
    table = _fisheye_lens_table(fn, lenses, len(srcs))
    cam = _camera_rows(ts, (0, 1, 2), B, dev, mode).contiguous()
    lens = torch.from_numpy(np.ascontiguousarray(table[idx], dtype=np.float32)).to(dev)
    srcs = [p.contiguous() for p in srcs]
    img = torch.empty((B, H, W, 3), dtype=srcs[0].dtype, device=dev)
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if return_mask else None
    p_src, hw, c_idx = _source_arrays(srcs, [(int(p.shape[0]), int(p.shape[1])) for p in srcs], idx)
    lib = load_library()
    with torch.cuda.device(dev):
        _check(lib.pf_fisheye_crop(dev.index, len(srcs), p_src, hw, _PANO_DTYPES[srcs[0].dtype], kind, B, c_idx, lens.data_ptr(), cam.data_ptr(), H, W, fill,
                                   img.data_ptr(), valid.data_ptr() if return_mask else None, samples, _stream_ptr()), None, "pf_fisheye_crop")
    mask = (valid.view(torch.bool),) if return_mask else ()
    if not fields:
        return (img, None, None) + mask
    pinhole = not torch.is_tensor(xi) and np.ndim(xi) == 0 and float(xi) == 0.0   # fields_from_params' rule: the number 0 is the pinhole model
    rows = [t.expand(B) for t in ts]
    per_view = [fields_from_params(rows[0][i], rows[1][i], rows[3][i], rows[4][i], rows[5][i], height=H, width=W, mode=mode, device=dev,
                                   xi=0.0 if pinhole else rows[6][i]) for i in range(B)]
    return (img, torch.stack([u for u, _ in per_view]), torch.stack([l for _, l in per_view])) + mask


def fisheye_to_panorama(frames, lenses, *, height, width, roll=0.0, pitch=0.0, yaw=0.0, inverse=False, frame_index=None, projection="equidistant", mode="deg",
                        fields=False, samples=1, fill=0, return_mask=False):
    """Fisheye and dual-fisheye frames -> equirectangular panoramas on the GPU, turned on the way if angles are given: the two lenses of a 360
    degree camera are blended across their overlap, and a tilted rig is levelled into a panorama in one pass.  Lens model and sampling:
    include/pf_hip.h pf_fisheye_to_pano.

    frames, lenses, projection, frame_index, fill: as `crop_fisheye`.  roll, pitch, yaw, inverse, mode, samples: `rotate_panorama`'s, with the
    frame in the place of the source panorama (inverse=False: what a panoramic camera with that orientation among the lenses sees;
    inverse=True: a frame shot by a rig with that orientation becomes upright).  height, width: the size of every output.
    Returns the images (B, H, W, 3) in the frames' dtype; with fields=True (images, up, lat), the fields being `panorama_fields(roll, pitch)`;
    with return_mask=True the mask (B, H, W) bool comes last: False where no lens covers the pixel, which then holds `fill`.  Non-finite angles
    give an image of `fill`.  GPU only: CPU frames raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    fn = "fisheye_to_panorama"
    samples = _check_samples(fn, samples)
    kind = _fisheye_kind(fn, projection)
    srcs, dev = _fisheye_frames(fn, frames)
    H, W = int(height), int(width)
    if H < 1 or W < 1:
        raise ValueError(f"output size must be at least 1 x 1; got {H} x {W}")
    if mode not in ("deg", "rad"):
        raise ValueError("mode must be 'deg' or 'rad'")
    fill = float(fill)
    ts = _rotation_params(fn, (("roll", roll), ("pitch", pitch), ("yaw", yaw)))
    B = _broadcast_len(fn, ts)
    if B < 1:
        raise ValueError(f"{fn} needs at least one output")
    idx = _frame_index(frame_index, B, len(srcs), "outputs")
    table = _fisheye_lens_table(fn, lenses, len(srcs))
    rot = _camera_rows(ts, (0, 1, 2), B, dev, mode).contiguous()
    lens = torch.from_numpy(np.ascontiguousarray(table[idx], dtype=np.float32)).to(dev)
    srcs = [p.contiguous() for p in srcs]
    img = torch.empty((B, H, W, 3), dtype=srcs[0].dtype, device=dev)
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if return_mask else None
    p_src, hw, c_idx = _source_arrays(srcs, [(int(p.shape[0]), int(p.shape[1])) for p in srcs], idx)
    lib = load_library()
    with torch.cuda.device(dev):
        _check(lib.pf_fisheye_to_pano(dev.index, len(srcs), p_src, hw, _PANO_DTYPES[srcs[0].dtype], kind, B, c_idx, lens.data_ptr(), rot.data_ptr(),
                                      1 if inverse else 0, H, W, fill, img.data_ptr(), valid.data_ptr() if return_mask else None, samples, _stream_ptr()),
               None, "pf_fisheye_to_pano")
    out = (img,)
    if fields:
        out += tuple(panorama_fields(ts[0].expand(B), ts[1].expand(B), height=H, width=W, mode=mode, device=dev))
    if return_mask:
        out += (valid.view(torch.bool),)
    return out[0] if len(out) == 1 else out


def panorama_to_cubemap(pano, size, *, roll=0.0, pitch=0.0, yaw=0.0, samples=1):
    """Equirectangular panoramas -> cube maps on the GPU: the six `crop_panorama` views of `cubemap_face_cameras()` at size x size, bit for bit.
    pano: a CUDA tensor (Hp, Wp, 3), uint8 or float32, or a list of B of them.  roll, pitch, yaw (degrees; numbers or B values): when one is given the
    panorama is first turned by `rotate_panorama` with these angles (the cube of a rig with that orientation inside the panorama), one more
    bilinear resampling.  samples: `crop_panorama`'s antialiasing of the faces.  Returns (B, 6, N, N, 3) in the panorama's dtype, faces front, right,
    back, left, up, down.  GPU only: CPU panoramas raise PfError."""
    fn = "panorama_to_cubemap"
    samples = _check_samples(fn, samples)
    panos, _ = _cuda_image_list(fn, [pano] if torch.is_tensor(pano) else list(pano), ("panorama", "panoramas"),
                                "a panorama must be (Hp, Wp, 3) with Hp, Wp >= 2", 2)
    N = operator.index(size)
    if N < 1:
        raise ValueError(f"{fn}: size must be at least 1; got {N}")
    ts = _rotation_params(fn, (("roll", roll), ("pitch", pitch), ("yaw", yaw)))
    B = len(panos)
    if _broadcast_len(fn, ts) not in (1, B) or any(t.dim() == 1 and t.shape[0] not in (1, B) for t in ts):
        raise ValueError(f"{fn}: roll, pitch and yaw are numbers or one value per panorama ({B})")
    if any(torch.is_tensor(v) or np.any(np.asarray(v) != 0) for v in (roll, pitch, yaw)):
        panos = [rotate_panorama(p, *(t if t.dim() == 0 else t[i % t.shape[0]] for t in ts))[0] for i, p in enumerate(panos)]
    cams = cubemap_face_cameras()
    faces, _, _ = crop_panorama(panos, cams["roll"] * B, cams["pitch"] * B, cams["rel_focal"] * B, yaw=cams["yaw"] * B, height=N, width=N,
                                pano_index=[i for i in range(B) for _ in range(6)], fields=False, samples=samples)
    return faces.view(B, 6, N, N, 3)


def _cube_layout(fn, layout):
    if layout not in ("strip", "cross"):
        raise ValueError(f"{fn}: layout must be 'strip' or 'cross'; got {layout!r}")


def cubemap_to_image(cube, layout):
    """A cube map (..., 6, N, N, 3) as one picture in an on-disk layout, by slicing alone (any device, any dtype): "strip" (..., N, 6 N, 3), faces
    0 ... 5 left to right; "cross" (..., 3 N, 4 N, 3), up at block (row 0, column 1), left, front, right, back at (1, 0 ... 3), down at (2, 1), the
    rest 0.  `cubemap_from_image` is the exact inverse."""
    fn = "cubemap_to_image"
    _cube_layout(fn, layout)
    if not torch.is_tensor(cube) or cube.dim() < 4 or cube.shape[-4] != 6 or cube.shape[-1] != 3 or cube.shape[-2] != cube.shape[-3] or cube.shape[-2] < 1:
        raise ValueError(f"{fn}: a cube map is a tensor (..., 6, N, N, 3) with N >= 1; got {tuple(cube.shape) if torch.is_tensor(cube) else type(cube)}")
    N = cube.shape[-2]
    if layout == "strip":
        return torch.cat([cube[..., k, :, :, :] for k in range(6)], dim=-2)
    img = cube.new_zeros(tuple(cube.shape[:-4]) + (3 * N, 4 * N, 3))
    for k, (br, bc) in enumerate(_CUBE_CROSS):
        img[..., br * N:(br + 1) * N, bc * N:(bc + 1) * N, :] = cube[..., k, :, :, :]
    return img


def cubemap_from_image(img, layout):
    """The cube map (..., 6, N, N, 3) of a picture (..., H, W, 3) in the layout "strip" (W = 6 H) or "cross" (H = 3 N, W = 4 N): `cubemap_to_image`'s
    inverse, by slicing alone; the blocks of a cross that hold no face are ignored."""
    fn = "cubemap_from_image"
    _cube_layout(fn, layout)
    if not torch.is_tensor(img) or img.dim() < 3 or img.shape[-1] != 3:
        raise ValueError(f"{fn}: a picture is a tensor (..., H, W, 3); got {tuple(img.shape) if torch.is_tensor(img) else type(img)}")
    H, W = img.shape[-3], img.shape[-2]
    if layout == "strip":
        if H < 1 or W != 6 * H:
            raise ValueError(f"{fn}: a strip is (N, 6 N, 3); got {H} x {W}")
        return torch.stack([img[..., :, k * H:(k + 1) * H, :] for k in range(6)], dim=-4)
    N = H // 3
    if N < 1 or H != 3 * N or W != 4 * N:
        raise ValueError(f"{fn}: a cross is (3 N, 4 N, 3); got {H} x {W}")
    return torch.stack([img[..., br * N:(br + 1) * N, bc * N:(bc + 1) * N, :] for br, bc in _CUBE_CROSS], dim=-4)


def _rot_roll_pitch(roll, pitch):
    """R = R_pitch(pitch) R_roll(roll), camera -> world, for fp64 tensors (..., ) of radians -> (..., 3, 3)"""
    cr, sr, cp, sp = torch.cos(roll), torch.sin(roll), torch.cos(pitch), torch.sin(pitch)
    z = torch.zeros_like(cr)
    return torch.stack([torch.stack([cr, -sr, z], -1), torch.stack([cp * sr, cp * cr, -sp], -1), torch.stack([sp * sr, sp * cr, cp], -1)], -2)


def _rot_yaw(yaw):
    """Y(yaw), the turn about y that adds yaw to the longitude"""
    c, s = torch.cos(yaw), torch.sin(yaw)
    z, o = torch.zeros_like(c), torch.ones_like(c)
    return torch.stack([torch.stack([c, z, s], -1), torch.stack([z, o, z], -1), torch.stack([-s, z, c], -1)], -2)


def gravity_from_views(view_cams, roll, pitch, *, weights=None, max_dev=15.0, mode="deg"):
    """The roll and pitch of a panorama from what was said about views cut out of it: every view's up direction, carried into the panorama's frame
    and averaged robustly.  Pure torch in fp64 on the device of its inputs (CPU or GPU); no host synchronisation.

    view_cams: a dict of the per-view `roll`, `pitch`, `yaw` with which the views were cut from one panorama (`crop_panorama`'s arguments; absent
    entries count as 0).  roll, pitch: what the model (pred_roll, pred_pitch) or `fit_camera` said about each view, N values.  Angles in degrees
    unless mode="rad"; max_dev and the returned `angles` are always degrees.
    View i votes v_i = V_i R(roll_i, pitch_i)^T (0, -1, 0) with V_i = Y(yaw_i) R(view roll_i, view pitch_i): the world's up in the panorama's
    frame.  The result is the weighted mean direction (weights: N values >= 0, default 1), re-averaged once over the views within max_dev
    degrees of it, and returned as the (roll, pitch) with R(roll, pitch)^T (0, -1, 0) = that direction -- what
    `rotate_panorama(pano, roll, pitch, inverse=True)` levels the panorama with.  A view with a non-finite prediction, camera or weight does not vote;
    without a voting view the result is NaN.
    Returns a dict: roll, pitch (0-d, in `mode` units), direction (3,), votes (N, 3; NaN rows for views that do not vote), inliers (N,) bool,
    angles (N,) degrees between each vote and the result."""
    if not isinstance(view_cams, Mapping):
        raise TypeError(f"gravity_from_views: view_cams must be a dict of roll, pitch, yaw; got {type(view_cams).__name__}")
    unknown = [k for k in view_cams if k not in ("roll", "pitch", "yaw")]
    if unknown:
        raise ValueError(f"gravity_from_views: view_cams may hold roll, pitch and yaw; unknown {unknown}")
    if mode not in ("deg", "rad"):
        raise ValueError("mode must be 'deg' or 'rad'")
    if not (float(max_dev) > 0.0):
        raise ValueError("max_dev must be > 0 degrees")
    named = [("view roll", view_cams.get("roll", 0.0)), ("view pitch", view_cams.get("pitch", 0.0)), ("view yaw", view_cams.get("yaw", 0.0)),
             ("roll", roll), ("pitch", pitch), ("weights", 1.0 if weights is None else weights)]
    ts = _rotation_params("gravity_from_views", named)
    N = _broadcast_len("gravity_from_views", ts)
    if N < 1:
        raise ValueError("gravity_from_views needs at least one view")
    dev = next((t.device for t in ts if t.device.type != "cpu"), torch.device("cpu"))
    ts = [t.to(device=dev, dtype=torch.float64).expand(N) for t in ts]
    vr, vp, vy, r, p = [torch.deg2rad(t) if mode == "deg" else t for t in ts[:5]]
    w = ts[5]
    up = torch.tensor([0.0, -1.0, 0.0], dtype=torch.float64, device=dev)
    votes = (_rot_yaw(vy) @ _rot_roll_pitch(vr, vp) @ _rot_roll_pitch(r, p).transpose(-1, -2)) @ up
    voting = torch.isfinite(votes).all(-1) & torch.isfinite(w) & (w >= 0)
    v0 = torch.where(voting[:, None], votes, torch.zeros_like(votes))
    w0 = torch.where(voting, w, torch.zeros_like(w))

    def mean_dir(wk):
        s = (wk[:, None] * v0).sum(0)
        return s / torch.linalg.vector_norm(s)   # 0 / 0 = NaN without a voting view

    def angles_to(d):
        return torch.rad2deg(torch.atan2(torch.linalg.vector_norm(torch.linalg.cross(votes, d.expand_as(votes)), dim=-1), votes @ d))

    first = mean_dir(w0)
    near = voting & (angles_to(first) <= float(max_dev))
    d = mean_dir(torch.where(near, w0, torch.zeros_like(w0)))
    d = torch.where(torch.isfinite(d).all(), d, first)   # no view within max_dev of the first mean: it stands
    ang = angles_to(d)
    # R(roll, pitch)^T (0, -1, 0) = (-cos p sin r, -cos p cos r, sin p)
    out_pitch = torch.atan2(d[2], torch.linalg.vector_norm(d[:2]))
    out_roll = torch.atan2(-d[0], -d[1])
    if mode == "deg":
        out_roll, out_pitch = torch.rad2deg(out_roll), torch.rad2deg(out_pitch)
    return {"roll": out_roll, "pitch": out_pitch, "direction": d, "votes": votes, "inliers": voting & (ang <= float(max_dev)), "angles": ang}


_CAM_KEYS = ("roll", "pitch", "yaw", "rel_focal", "rel_cx", "rel_cy", "xi")   # the row order of pf_reproject's d_cam_src7 / d_cam_dst7
_CAM_REQUIRED = ("roll", "pitch", "rel_focal")


def _camera_params(what, cam, fn="reproject_image"):
    """a camera dict -> its seven values as tensors in the order of _CAM_KEYS, checked where they are (nothing moves to the device yet)"""
    if not isinstance(cam, Mapping):
        raise TypeError(f"{fn}: {what} must be a dict of camera parameters; got {type(cam).__name__}")
    unknown = [k for k in cam if k not in _CAM_KEYS]
    missing = [k for k in _CAM_REQUIRED if k not in cam]
    if unknown or missing:
        raise ValueError(f"{fn}: {what} needs {_CAM_REQUIRED} and may hold {_CAM_KEYS[2:3] + _CAM_KEYS[4:]}; unknown {unknown}, missing {missing}")
    ts = []
    for k in _CAM_KEYS:
        v = cam.get(k, 0.0)
        t = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.float64))
        if t.dim() > 1:
            raise ValueError(f"{what}[{k!r}] must be a number or a 1-d sequence; got shape {tuple(t.shape)}")
        ts.append(t)
    return ts


def reproject_image(images, src, dst, *, height=None, width=None, src_index=None, mode="deg", fill=0, return_valid=False, return_map=False, samples=1):
    """Images of one camera -> images of another camera of the same centre on the GPU: upright rectification (destination roll 0, or roll
    and pitch 0), undistortion of a Unified Spherical Model view (destination xi = 0), another focal length, principal point or output
    size, or any other view of the same centre.  Model: include/pf_hip.h pf_reproject; the cameras are those of
    `crop_panorama` and `fields_from_params`, so the perspective fields of the result are `fields_from_params` of `dst`.

    images: a CUDA tensor (Hs, Ws, 3) or (B, Hs, Ws, 3), uint8 or float32, or a list of (Hs, Ws, 3) tensors of one dtype and one device,
    whose sizes may differ.  src, dst: dicts with `roll`, `pitch`, `rel_focal` (required) and `yaw`, `rel_cx`, `rel_cy`, `xi` (default 0);
    angles in degrees unless mode="rad"; each value a number, a 0-d tensor or a 1-d sequence / tensor, broadcast to the batch size B;
    device tensors stay on the device.  src describes the camera that took the image, dst the camera to render.
    B and the source of each output: with src_index (B integers into the images) B = len(src_index); otherwise one output per image, or,
    for a single image, as many as the parameters broadcast to.  height, width: the size of every output; default: the size of the
    sources (a ValueError when they differ).  fill: the value of the pixels that see nothing of their source (no ray, behind the
    source camera, outside its image).
    Returns the images (B, H, W, 3) in the sources' dtype; with return_valid / return_map a tuple that adds the mask (B, H, W) bool and /
    or the map (B, 2, H, W) float32 of source coordinates (a_s, b_s) in pixel-edge units (NaN where the source camera does not see the ray).
    Bilinear sampling without mip levels; samples=S (1 .. 4) antialiases an output that minifies its source: every pixel is the mean of the valid
    ones of S x S bilinear sub-samples (include/pf_hip.h pf_reproject_ss).  The mask is then True where any sub-sample is valid
    (the pixels outside it, and only those, were given `fill`), and the map stays the pixel centre's.  GPU only: CPU images raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    samples = _check_samples("reproject_image", samples)

    batched = torch.is_tensor(images) and images.dim() == 4   # (B, Hs, Ws, 3): only as one tensor, not inside a list
    srcs = [] if batched and images.shape[0] < 1 else [images] if torch.is_tensor(images) else list(images)
    srcs, dev = _cuda_image_list("reproject_image", srcs, ("image", "images"), "an image must be (Hs, Ws, 3) with Hs, Ws >= 1, or a tensor (B, Hs, Ws, 3)", 1,
                                 ndim=4 if batched else 3)
    n = int(srcs[0].shape[0]) if batched else len(srcs)
    sizes = [(int(srcs[0].shape[1]), int(srcs[0].shape[2]))] * n if batched else [(int(p.shape[0]), int(p.shape[1])) for p in srcs]
    if height is None or width is None:
        if len(set(sizes)) != 1:
            raise ValueError("reproject_image: the images differ in size; give height and width")
    H = sizes[0][0] if height is None else int(height)
    W = sizes[0][1] if width is None else int(width)
    if H < 1 or W < 1:
        raise ValueError(f"output size must be at least 1 x 1; got {H} x {W}")
    if mode not in ("deg", "rad"):
        raise ValueError("mode must be 'deg' or 'rad'")
    fill = float(fill)
    ts = _camera_params("src", src) + _camera_params("dst", dst)
    Bp = _broadcast_len("reproject_image", ts)
    if src_index is not None:
        idx = [operator.index(i) for i in (src_index.tolist() if torch.is_tensor(src_index) else src_index)]
        if any(i < 0 or i >= n for i in idx):
            raise ValueError(f"src_index entries must be in [0, {n})")
    else:
        idx = list(range(n)) if n > 1 else [0] * Bp
    B = len(idx)
    if B < 1:
        raise ValueError("reproject_image needs at least one output")
    if Bp not in (1, B):
        raise ValueError(f"reproject_image: camera parameters of length {Bp} for {B} outputs")
    cam = _camera_rows(ts, (0, 1, 2, 7, 8, 9), B, dev, mode)
    cam_s, cam_d = cam[:, :7].contiguous(), cam[:, 7:].contiguous()
    if batched:
        whole = srcs[0].contiguous()
        srcs = [whole[i] for i in range(n)]
    else:
        srcs = [p.contiguous() for p in srcs]
    img = torch.empty((B, H, W, 3), dtype=srcs[0].dtype, device=dev)
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if return_valid else None
    cmap = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev) if return_map else None
    p_src, hw, c_idx = _source_arrays(srcs, sizes, idx)
    lib = load_library()
    with torch.cuda.device(dev):
        args = (dev.index, n, p_src, hw, _PANO_DTYPES[srcs[0].dtype], B, c_idx, cam_s.data_ptr(), cam_d.data_ptr(), H, W, fill,
                img.data_ptr(), valid.data_ptr() if return_valid else None, cmap.data_ptr() if return_map else None)
        if samples == 1:
            _check(lib.pf_reproject(*args, _stream_ptr()), None, "pf_reproject")
        else:
            _check(lib.pf_reproject_ss(*args, samples, _stream_ptr()), None, "pf_reproject_ss")
    out = (img,) + ((valid.view(torch.bool),) if return_valid else ()) + ((cmap,) if return_map else ())
    return out[0] if len(out) == 1 else out


DRAW_UP, DRAW_LAT = 1, 2   # include/pf_hip.h PF_DRAW_*


def _draw_images(fn, images):
    """the pictures of a drawing call -> (kind, list as given): 'single' (H, W, 3), 'batched' (B, H, W, 3) or 'list'"""
    if torch.is_tensor(images):
        return ("batched", [images]) if images.dim() == 4 else ("single", [images])
    if not isinstance(images, (list, tuple)):
        raise TypeError(f"{fn} takes a torch tensor or a list of them as images")
    return "list", list(images)


def draw_perspective_fields(images, up, lat, *, density=10, arrow_inv_len=20, lat_step_deg=10.0, alpha=0.5, arrow_color=(0, 255, 0), line_width=1.0,
                            draw_up=True, draw_lat=True, out=None):
    """Perspective fields drawn over their pictures on the GPU, the first look at a prediction: a latitude tint (a diverging colour ramp, light at
    the horizon), iso-latitude lines every lat_step_deg degrees (the horizon twice as wide) and a grid of green arrows along the up vectors.  The
    drawing model is this library's own -- include/pf_hip.h pf_draw_fields -- and not matplotlib's rasteriser.

    images: a CUDA tensor (H, W, 3) or (B, H, W, 3), uint8 or float32 on the 0 - 255 scale, or a list of (H, W, 3) tensors of one dtype and one
    device whose sizes may differ.  up (2, H, W) and lat (H, W) degrees, the layout of `pred_gravity_original` / `pred_latitude_original`: one
    pair, batched tensors or lists, one pair per image and of its image's size (resizing fields is the caller's job).  A pixel with a non-finite
    field value or an up vector shorter than 1e-6 is not drawn on: NaN is the mask.
    density: arrows along the shorter side (the anchors are s = max(1, min(H, W) // density) pixels apart); arrow_inv_len: an arrow is
    W / arrow_inv_len pixels long; alpha: opacity of the tint; arrow_color: RGB on the 0 - 255 scale; line_width: of lines and arrows, pixels;
    draw_up / draw_lat switch the arrows / the tint and the lines.  out: where to draw, of the images' type and shapes (the images themselves
    are allowed); default: new tensors.
    Returns what was given: a tensor (H, W, 3), a tensor (B, H, W, 3) or a list.  uint8 results are rounded half up.  One C call for all images
    whose spacing s is the same -- one call for images of one size -- on the current stream, without a host synchronisation.  Deterministic; a
    picture's bits do not depend on the batch it is in.  GPU only: CPU tensors raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    fn = "draw_perspective_fields"
    kind, ims = _draw_images(fn, images)
    _, ups, lats = _field_list("the", up, lat, fn)
    # the checks that need no device, in the caller's terms, before anything is looked at on a device
    density, arrow_inv_len, lat_step_deg, alpha, line_width = operator.index(density), float(arrow_inv_len), float(lat_step_deg), float(alpha), float(line_width)
    if density < 1:
        raise ValueError(f"density must be at least 1; got {density}")
    if not (arrow_inv_len > 0.0 and np.isfinite(arrow_inv_len) and 1.0 / arrow_inv_len <= 1e6):
        raise ValueError(f"arrow_inv_len must be finite and > 0 (at least 1e-6); got {arrow_inv_len}")
    if not (lat_step_deg > 0.0 and np.isfinite(lat_step_deg)):
        raise ValueError(f"lat_step_deg must be finite and > 0; got {lat_step_deg}")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must be in [0, 1]; got {alpha}")
    if not (line_width >= 0.0 and np.isfinite(line_width)):
        raise ValueError(f"line_width must be finite and >= 0; got {line_width}")
    rgb = [float(c) for c in arrow_color]
    if len(rgb) != 3 or not all(np.isfinite(c) for c in rgb):
        raise ValueError(f"arrow_color must be three finite numbers; got {arrow_color}")
    if not all(torch.is_tensor(t) for t in ims + ups + lats):
        raise TypeError(f"{fn} takes torch tensors")
    shapes = [tuple(im.shape[1:3]) for im in ims for _ in range(im.shape[0])] if kind == "batched" else [tuple(im.shape[:2]) for im in ims]
    if len(ups) != len(shapes):
        raise ValueError(f"{fn}: {len(ups)} fields for {len(shapes)} images")
    for hw, u, l in zip(shapes, ups, lats):
        if u.dim() != 3 or u.shape[0] != 2 or tuple(l.shape) != tuple(u.shape[1:]):
            raise ValueError(f"up must be (2, H, W) and lat (H, W); got {tuple(u.shape)} and {tuple(l.shape)}")
        if tuple(l.shape) != hw:
            raise ValueError(f"{fn}: fields of size {tuple(l.shape)} for an image of size {hw}: the fields must have the size of their image")
    ims, dev = _cuda_image_list(fn, [] if kind == "batched" and ims[0].shape[0] < 1 else ims, ("image", "images"),
                                "an image must be (H, W, 3) with H, W >= 1, or a tensor (B, H, W, 3)", 1, ndim=4 if kind == "batched" else 3)
    if not all(t.is_cuda for t in ups + lats):
        raise PfError(f"{fn} runs on the GPU only (no CPU path)")
    if any((t.device if t.device.index is not None else torch.device("cuda", torch.cuda.current_device())) != dev for t in ups + lats):
        raise ValueError(f"{fn}: images and fields must be on one device")
    if out is not None:
        _, outs = _draw_images(fn, out)
        if len(outs) != len(ims) or any(not torch.is_tensor(o) or o.shape != im.shape or o.dtype != im.dtype or o.device != im.device or not o.is_contiguous()
                                       for o, im in zip(outs, ims)):
            raise ValueError(f"{fn}: out must be contiguous and of the images' type, shapes and device")
    ims = [im.contiguous() for im in ims]
    outs = [torch.empty_like(im) for im in ims] if out is None else outs
    if kind == "batched":
        src, dst = list(ims[0].unbind(0)), list(outs[0].unbind(0))
    else:
        src, dst = ims, outs
    ups, lats = ([t.to(torch.float32).contiguous() for t in ts] for ts in (ups, lats))
    layers = (DRAW_UP if draw_up else 0) | (DRAW_LAT if draw_lat else 0)
    groups = OrderedDict()   # spacing -> images: the C call takes one spacing
    for i, (h, w) in enumerate(shapes):
        groups.setdefault(max(1, min(h, w) // density), []).append(i)
    c_rgb = (ctypes.c_float * 3)(*rgb)
    lib = load_library()
    with torch.cuda.device(dev):
        for spacing, idx in groups.items():
            n = len(idx)
            ptrs = lambda ts: (ctypes.c_void_p * n)(*[ts[i].data_ptr() for i in idx])
            hw = (ctypes.c_int32 * (2 * n))(*[s for i in idx for s in shapes[i]])
            need = int(lib.pf_draw_fields_workspace_bytes(n, hw, spacing))
            if need == 0:
                raise ValueError(f"{fn}: image sizes that one call does not take (2^31 pixels or more)")
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            _check(lib.pf_draw_fields(dev.index, n, hw, ptrs(src), ptrs(ups), ptrs(lats), ptrs(dst), _PANO_DTYPES[src[0].dtype], spacing, 1.0 / arrow_inv_len,
                                      lat_step_deg, alpha, line_width, c_rgb, layers, ws.data_ptr(), need, _stream_ptr()), None, "pf_draw_fields")
    return outs if kind == "list" else outs[0]


def draw_camera(images, roll, pitch, rel_focal, rel_cx=0.0, rel_cy=0.0, *, xi=0.0, mode="deg", **kw):
    """The perspective fields of a camera drawn over pictures on the GPU: `fields_from_params` for every image's size, then
    `draw_perspective_fields` (whose options -- density, arrow_inv_len, lat_step_deg, alpha, arrow_color, line_width, draw_up, draw_lat, out --
    pass through); the reference's draw_from_r_p_f_cx_cy with the focal length given directly.  images as there.  roll, pitch (degrees unless
    mode="rad"), rel_focal, rel_cx, rel_cy, xi: numbers or 0-d tensors for all images, or 1-d sequences / tensors of one value per image."""
    fn = "draw_camera"
    kind, ims = _draw_images(fn, images)
    ims, dev = _cuda_image_list(fn, [] if kind == "batched" and torch.is_tensor(ims[0]) and ims[0].shape[0] < 1 else ims, ("image", "images"),
                                "an image must be (H, W, 3) with H, W >= 1, or a tensor (B, H, W, 3)", 1, ndim=4 if kind == "batched" else 3)
    shapes = [tuple(im.shape[1:3]) for im in ims for _ in range(im.shape[0])] if kind == "batched" else [tuple(im.shape[:2]) for im in ims]

    def pick(name, v, i):
        if isinstance(v, (list, tuple, np.ndarray)) or (torch.is_tensor(v) and v.dim() == 1):
            if len(v) != len(shapes):
                raise ValueError(f"{fn}: {len(v)} values of {name} for {len(shapes)} images")
            return v[i]
        return v

    params = (("roll", roll), ("pitch", pitch), ("rel_focal", rel_focal), ("rel_cx", rel_cx), ("rel_cy", rel_cy))
    fields = [fields_from_params(*[pick(k, v, i) for k, v in params], height=h, width=w, mode=mode, device=dev, xi=pick("xi", xi, i))
              for i, (h, w) in enumerate(shapes)]
    ups, lats = [f[0] for f in fields], [f[1] for f in fields]
    return draw_perspective_fields(images, ups[0] if kind == "single" else ups, lats[0] if kind == "single" else lats, **kw)


BLEND_FEATHER, BLEND_MEAN = 0, 1
_BLENDS ={"feather": BLEND_FEATHER, "mean": BLEND_MEAN}
_COMPOSE_MAX_VIEWS = 32   # views of one panorama per launch (csrc/pf_kernels.h ComposeBatch::MAX); more need the accumulator


def compose_panorama(images, cams, *, height, width, pano_index=None, n_pano=None, blend="feather", mode="deg", fill=0, return_weight=False):
    """Camera views of one centre -> equirectangular panoramas on the GPU: the inverse direction of `crop_panorama`, with several views
    blended per panorama pixel.  Model: include/pf_hip.h pf_pano_compose; the cameras and the panorama's
    longitude / latitude convention are those of `crop_panorama`, so composing its crops gives the panorama back where they cover it.

    images: what `reproject_image` takes -- a CUDA tensor (Hs, Ws, 3) or (B, Hs, Ws, 3), uint8 or float32, or a list of (Hs, Ws, 3) tensors of
    one dtype and one device, whose sizes may differ.  cams: a dict with `roll`, `pitch`, `rel_focal` (required) and `yaw`, `rel_cx`,
    `rel_cy`, `xi` (default 0); angles in degrees unless mode="rad"; each value a number, a 0-d tensor or a 1-d sequence / tensor of one
    entry per view; device tensors stay on the device.
    height, width: the size Hp x Wp of every panorama.  pano_index: None (one panorama from all views) or one integer per view, the panorama
    it belongs to; the views are sorted by it on the host, stably, so the blend order within a panorama is the caller's.  n_pano: the
    number of panoramas, default max(pano_index) + 1; a panorama without views is all `fill`.
    blend: "feather" -- a view's weight falls linearly from 1 in the middle of its short side to 0 on its border, so the composite is
    continuous across view borders; "mean" -- every covering view counts the same (one view: its bilinear sample).  fill: the value of
    the pixels that no view covers.
    Returns the panoramas (n_pano, Hp, Wp, 3) in the views' dtype; with return_weight=True also the summed weight (n_pano, Hp, Wp)
    float32, 0 where nothing covers the pixel.  Bilinear sampling without antialiasing: a strongly minified view aliases.
    GPU only: CPU images raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    batched = torch.is_tensor(images) and images.dim() == 4
    srcs = [] if batched and images.shape[0] < 1 else [images] if torch.is_tensor(images) else list(images)
    srcs, dev = _cuda_image_list("compose_panorama", srcs, ("view", "views"), "a view must be (Hs, Ws, 3) with Hs, Ws >= 1, or a tensor (B, Hs, Ws, 3)", 1,
                                 ndim=4 if batched else 3)
    n = int(srcs[0].shape[0]) if batched else len(srcs)
    sizes = [(int(srcs[0].shape[1]), int(srcs[0].shape[2]))] * n if batched else [(int(p.shape[0]), int(p.shape[1])) for p in srcs]
    Hp, Wp = int(height), int(width)
    if Hp < 1 or Wp < 1:
        raise ValueError(f"panorama size must be at least 1 x 1; got {Hp} x {Wp}")
    if mode not in ("deg", "rad"):
        raise ValueError("mode must be 'deg' or 'rad'")
    if blend not in _BLENDS:
        raise ValueError(f"blend must be one of {tuple(_BLENDS)}; got {blend!r}")
    fill = float(fill)
    ts = _camera_params("cams", cams, "compose_panorama")
    Bp = _broadcast_len("compose_panorama", ts)
    if Bp not in (1, n):
        raise ValueError(f"compose_panorama: camera parameters of length {Bp} for {n} views")
    if pano_index is None:
        idx = [0] * n
    else:
        idx = [operator.index(i) for i in (pano_index.tolist() if torch.is_tensor(pano_index) else pano_index)]
        if len(idx) != n:
            raise ValueError(f"pano_index has {len(idx)} entries for {n} views")
        if any(i < 0 for i in idx):
            raise ValueError("pano_index entries must be >= 0")
    P = max(idx) + 1 if n_pano is None else operator.index(n_pano)
    if P < 1 or any(i >= P for i in idx):
        raise ValueError(f"pano_index entries must be in [0, {P}) (n_pano)")
    order = sorted(range(n), key=idx.__getitem__)   # stable: the caller's order within a panorama
    cam = _camera_rows(ts, (0, 1, 2), n, dev, mode)
    if order != list(range(n)):
        cam = cam[torch.as_tensor(order, device=dev)]
    cam = cam.contiguous()
    if batched:
        whole = srcs[0].contiguous()
        srcs = [whole[i] for i in range(n)]
    else:
        srcs = [p.contiguous() for p in srcs]
    srcs = [srcs[i] for i in order]
    counts = [0] * P
    for i in idx:
        counts[i] += 1
    pano = torch.empty((P, Hp, Wp, 3), dtype=srcs[0].dtype, device=dev)
    weight = torch.empty((P, Hp, Wp), dtype=torch.float32, device=dev) if return_weight else None
    acc = torch.empty((P, Hp, Wp, 4), dtype=torch.float32, device=dev) if max(counts) > _COMPOSE_MAX_VIEWS else None
    p_src, hw, c_idx = _source_arrays(srcs, [sizes[i] for i in order], [idx[i] for i in order])
    lib = load_library()
    with torch.cuda.device(dev):
        _check(lib.pf_pano_compose(dev.index, n, p_src, hw, _PANO_DTYPES[srcs[0].dtype], c_idx, cam.data_ptr(), P, Hp, Wp, _BLENDS[blend], fill,
                                   pano.data_ptr(), weight.data_ptr() if return_weight else None, acc.data_ptr() if acc is not None else None,
                                   _stream_ptr()), None, "pf_pano_compose")
    return (pano, weight) if return_weight else pano


_YAW_MAX_CAND = 4096   # include/pf_hip.h PF_YAW_MAX_CAND
_YAW_CAM_COLS = (0, 1, 3, 4, 5, 6)   # _CAM_KEYS without the yaw: the row order of pf_yaw_moments's d_cam6


def yaw_scores(images, cams, pairs, candidates, *, stride=None, min_overlap=0.1, mode="deg", return_moments=False):
    """How well the pictures of two views of one centre agree when the second is turned by a candidate angle about the vertical against the
    first, on the GPU.  Model: include/pf_hip.h pf_yaw_moments.

    images, cams: what `compose_panorama` takes (a `yaw` entry of cams is ignored).  pairs: a sequence of (a, b) view indices, a != b.
    candidates: the turns yaw_b - yaw_a to try, in degrees (also with mode="rad", which is about the cameras' angles), a 1-d sequence or
    tensor of at most 4096 entries.  stride: every stride-th row and column of b is a sample; default max(1, min(H, W) // 48) of the
    smallest view, one stride per call (a search in steps of 1 degree does not need more samples).
    Returns (score (P, K) float64, overlap (P, K) float64) on the device; with return_moments=True also the moments (P, K, 6) float64
    (n, sum x, sum y, sum x^2, sum y^2, sum xy of the luminances x of a and y of b over the covered samples).  score is the zero-mean
    normalised cross-correlation, in [-1, 1], computed from the moments in float64; it is -inf where fewer than min_overlap x (samples of b
    that have a ray) samples are covered or a variance is not positive (see _zncc).  overlap is the covered share of those samples.
    GPU only: CPU images raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    batched = torch.is_tensor(images) and images.dim() == 4
    srcs = [] if batched and images.shape[0] < 1 else [images] if torch.is_tensor(images) else list(images)
    srcs, dev = _cuda_image_list("yaw_scores", srcs, ("view", "views"), "a view must be (H, W, 3) with H, W >= 1, or a tensor (B, H, W, 3)", 1,
                                 ndim=4 if batched else 3)
    n = int(srcs[0].shape[0]) if batched else len(srcs)
    sizes = [(int(srcs[0].shape[1]), int(srcs[0].shape[2]))] * n if batched else [(int(p.shape[0]), int(p.shape[1])) for p in srcs]
    if n < 2:
        raise ValueError("yaw_scores needs at least two views")
    if mode not in ("deg", "rad"):
        raise ValueError("mode must be 'deg' or 'rad'")
    if stride is None:
        stride = max(1, min(min(hw) for hw in sizes) // 48)
    stride = operator.index(stride)
    if stride < 1:
        raise ValueError(f"stride must be at least 1; got {stride}")
    min_overlap = float(min_overlap)
    if not 0.0 <= min_overlap <= 1.0:
        raise ValueError(f"min_overlap must be in [0, 1]; got {min_overlap}")
    ts = _camera_params("cams", cams, "yaw_scores")
    Bp = _broadcast_len("yaw_scores", ts)
    if Bp not in (1, n):
        raise ValueError(f"yaw_scores: camera parameters of length {Bp} for {n} views")
    plist = [(operator.index(a), operator.index(b)) for a, b in (pairs.tolist() if torch.is_tensor(pairs) else pairs)]
    if not plist:
        raise ValueError("yaw_scores needs at least one pair")
    for a, b in plist:
        if not (0 <= a < n and 0 <= b < n) or a == b:
            raise ValueError(f"a pair is two different view indices in [0, {n}); got ({a}, {b})")
    cand = candidates if torch.is_tensor(candidates) else torch.as_tensor(np.asarray(candidates, dtype=np.float64))
    if cand.dim() != 1 or not 1 <= cand.shape[0] <= _YAW_MAX_CAND:
        raise ValueError(f"candidates must be a 1-d sequence of 1 to {_YAW_MAX_CAND} angles; got shape {tuple(cand.shape)}")
    P, K = len(plist), int(cand.shape[0])
    cam = _camera_rows(ts, (0, 1, 2), n, dev, mode)[:, list(_YAW_CAM_COLS)].contiguous()
    cand = torch.deg2rad(cand.to(device=dev, dtype=torch.float64)).to(torch.float32).contiguous()
    if batched:
        whole = srcs[0].contiguous()
        srcs = [whole[i] for i in range(n)]
    else:
        srcs = [p.contiguous() for p in srcs]
    p_src, hw, _ = _source_arrays(srcs, sizes, [0])
    c_pairs = (ctypes.c_int32 * (2 * P))(*[i for ab in plist for i in ab])
    lib = load_library()
    need = int(lib.pf_yaw_moments_workspace_bytes(n, hw, P, c_pairs, K, stride))
    if need == 0:
        raise ValueError("yaw_scores: the views, pairs and stride give more samples than one call takes")
    moments = torch.empty((P, K, 6), dtype=torch.float64, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib.pf_yaw_moments(dev.index, n, p_src, hw, _PANO_DTYPES[srcs[0].dtype], cam.data_ptr(), P, c_pairs, K, cand.data_ptr(), stride,
                                  moments.data_ptr(), ws.data_ptr(), need, _stream_ptr()), None, "pf_yaw_moments")
    # the samples of b that have a ray: disc >= 0 (include/pf_hip.h pf_reproject step 1), in float64 from the float32 rows the kernel reads
    cam64, rays = cam.to(torch.float64), torch.empty(n, dtype=torch.float64, device=dev)
    for H, W in sorted(set(sizes)):   # the views of one size together
        own = torch.as_tensor([i for i, hw in enumerate(sizes) if hw == (H, W)], device=dev)
        r = cam64[own]
        x = (torch.arange(0, W, stride, device=dev, dtype=torch.float64)[None, :] + 0.5 - ((r[:, 3] + 0.5) * W)[:, None]) / (r[:, 2] * H)[:, None]
        y = (torch.arange(0, H, stride, device=dev, dtype=torch.float64)[None, :] + 0.5 - ((r[:, 4] + 0.5) * H)[:, None]) / (r[:, 2] * H)[:, None]
        disc = 1.0 + (1.0 - r[:, 5] * r[:, 5])[:, None, None] * (x[:, None, :] ** 2 + y[:, :, None] ** 2)
        rays[own] = (disc >= 0).sum((1, 2)).to(torch.float64)
    rays = rays[torch.as_tensor([b for _, b in plist], device=dev)]
    score, overlap = _zncc(moments, rays, min_overlap)
    return (score, overlap, moments) if return_moments else (score, overlap)


def _zncc(moments, rays, min_overlap):
    """moments (P, K, 6) float64 and the samples with a ray (P,) -> (score, overlap) (P, K) float64: include/pf_hip.h pf_yaw_moments's ZNCC, -inf
    where n < min_overlap x rays or a variance is not positive (not above 2^-16 of n x its sum of squares: the sums are kept in float32 per
    tile, which cannot tell such a variance from 0; one covered sample, or a flat picture, has no score)"""
    n, sx, sy, sxx, syy, sxy = moments.unbind(-1)
    va, vb = n * sxx - sx * sx, n * syy - sy * sy
    ok = (n >= min_overlap * rays[:, None]) & (va > 2.0 ** -16 * n * sxx) & (vb > 2.0 ** -16 * n * syy)
    one = torch.ones_like(va)
    score = torch.where(ok, (n * sxy - sx * sy) / torch.sqrt(torch.where(ok, va, one) * torch.where(ok, vb, one)), torch.full_like(va, float("-inf")))
    overlap = torch.where(rays[:, None] > 0, n / torch.clamp(rays[:, None], min=1.0), torch.zeros_like(n))
    return score, overlap


def _wrap180(x):
    """degrees wrapped to [-180, 180)"""
    return (x + 180.0) % 360.0 - 180.0


def yaw_tree(delta, peak, *, anchor=0, min_score=0.8):
    """The yaws of N views from the tables of their ordered pairs, on the host (no GPU): delta[a, b] (degrees) is the measured turn
    yaw_b - yaw_a of the ordered pair (a, b) and peak[a, b] its score (the diagonal is ignored; -inf or NaN: no measurement).
    Of the two orders of a pair the one with the higher peak is kept (a tie keeps a < b) and the other order's turn is its negative.  A
    maximum spanning tree grows from `anchor` (Prim) over the pairs with a kept peak >= min_score; equal peaks go to the lower new view, then
    to the lower parent.  The anchor's yaw is 0, a child's is its parent's plus the turn, wrapped to [-180, 180).
    Returns (yaw (N,) float64 with NaN for the views the tree does not reach, parent (N,) int64 with -1 for the anchor and for those
    views, linked (N,) bool)."""
    delta, peak = np.asarray(delta, dtype=np.float64), np.asarray(peak, dtype=np.float64)
    N = delta.shape[0]
    if delta.shape != (N, N) or peak.shape != (N, N):
        raise ValueError(f"delta and peak must be square tables of one size; got {delta.shape} and {peak.shape}")
    anchor = operator.index(anchor)
    if not 0 <= anchor < N:
        raise ValueError(f"anchor must be in [0, {N}); got {anchor}")
    pk = np.where(np.isfinite(peak) & np.isfinite(delta), peak, -np.inf)
    w, turn = np.full((N, N), -np.inf), np.zeros((N, N))   # turn[u, v] = yaw_v - yaw_u of the kept order
    for a in range(N):
        for b in range(a + 1, N):
            fwd = pk[a, b] >= pk[b, a]
            w[a, b] = w[b, a] = pk[a, b] if fwd else pk[b, a]
            turn[a, b] = delta[a, b] if fwd else -delta[b, a]
            turn[b, a] = -turn[a, b]
    yaw, parent, linked = np.full(N, np.nan), np.full(N, -1, dtype=np.int64), np.zeros(N, dtype=bool)
    yaw[anchor], linked[anchor] = 0.0, True
    while True:
        best = None
        for v in range(N):
            if linked[v]:
                continue
            for u in range(N):
                if linked[u] and w[u, v] >= min_score and (best is None or w[u, v] > best[0]):
                    best = (w[u, v], v, u)
        if best is None:
            return yaw, parent, linked
        _, v, u = best
        yaw[v], parent[v], linked[v] = _wrap180(yaw[u] + turn[u, v]), u, True


def align_yaw(images, cams, *, anchor=0, step=1.0, stride=None, min_overlap=0.1, min_score=0.8, refine=True, mode="deg", return_info=False):
    """The yaw of every view of one centre, recovered from the pictures on the GPU: the one camera parameter the perspective fields do not
    carry, and what `compose_panorama` takes as `yaw`.  Model: include/pf_hip.h pf_yaw_moments.

    images, cams: what `compose_panorama` takes, N >= 2 views with their roll, pitch and intrinsics (a `yaw` entry is ignored).  Every ordered
    pair (a, b), a != b, is scored by `yaw_scores` (see there for stride and min_overlap) at the candidates -180 + k step, k < round(360 / step)
    degrees; its turn is the candidate with the highest score, with refine=True moved by the vertex of the parabola through that score and its
    two circular neighbours (not moved where a neighbour has no score).  `yaw_tree` then places the views: a maximum spanning tree from
    `anchor` over the pairs whose score reaches min_score.
    Returns yaw (N,) float64 in degrees on the device, in [-180, 180), 0 for the anchor and NaN for a view that no pair of sufficient score
    ties to the anchor's tree.  With return_info=True also a dict: `delta`, `peak`, `overlap` (N, N) float64 on the device, by ordered pair
    [a, b] (NaN, -inf, 0 on the diagonal), and `parent` (N,) int64, `linked` (N,) bool on the host.
    min_score = 0.8 lies between the scores of overlapping views of one scene (0.98 and more on the low-pass test scenes) and of views
    that do not overlap or show different scenes (0.58 and less there).  It is a default, not a guarantee: repetitive scenes can score
    high at a wrong turn, and strongly differing exposure, parallax or moving objects lower the score of a right one.
    GPU only: CPU images raise PfError."""
    step = float(step)
    if not (step > 0 and round(360.0 / step) >= 1 and round(360.0 / step) <= _YAW_MAX_CAND):
        raise ValueError(f"step must give 1 to {_YAW_MAX_CAND} candidates (360 / step); got {step}")
    min_score = float(min_score)
    n = int(images.shape[0]) if torch.is_tensor(images) and images.dim() == 4 else 1 if torch.is_tensor(images) else len(images)
    if n >= 2 and not 0 <= operator.index(anchor) < n:
        raise ValueError(f"anchor must be in [0, {n}); got {anchor}")
    K = int(round(360.0 / step))
    cand = -180.0 + step * np.arange(K, dtype=np.float64)
    pairs = [(a, b) for a in range(n) for b in range(n) if a != b]
    score, overlap = yaw_scores(images, cams, pairs, cand, stride=stride, min_overlap=min_overlap, mode=mode)
    dev = score.device
    peak, k = score.max(dim=1)
    delta = torch.as_tensor(cand, device=dev)[k]
    if refine and K >= 3:
        zm, zp = score.gather(1, ((k - 1) % K)[:, None])[:, 0], score.gather(1, ((k + 1) % K)[:, None])[:, 0]
        curv = zm - 2.0 * peak + zp
        ok = torch.isfinite(zm) & torch.isfinite(zp) & torch.isfinite(peak) & (curv < 0)
        delta = delta + step * torch.where(ok, 0.5 * (zm - zp) / torch.where(ok, curv, torch.ones_like(curv)), torch.zeros_like(curv))
    idx = torch.as_tensor(pairs, device=dev)
    tables = torch.zeros((3, n, n), dtype=torch.float64, device=dev)
    tables[0].fill_(float("nan"))
    tables[1].fill_(float("-inf"))
    tables[:, idx[:, 0], idx[:, 1]] = torch.stack([delta, peak, overlap.gather(1, k[:, None])[:, 0]])
    host = tables[:2].cpu().numpy()   # the one copy to the host
    yaw, parent, linked = yaw_tree(host[0], host[1], anchor=anchor, min_score=min_score)
    yaw = torch.as_tensor(yaw, device=dev)
    if return_info:
        return yaw, dict(delta=tables[0], peak=tables[1], overlap=tables[2], parent=parent, linked=linked)
    return yaw
