"""Host-side mirror of the reference's per-frame decode state for the VarDCT
back-end (PassesDecoderState + RenderPipeline, lib/jxl/dec_cache.h:86-229,
lib/jxl/render_pipeline/render_pipeline.h:139-152) on top of the C ABI.

PyTorch is plumbing only: it owns the HBM tensors and the stream; every
computation happens in libjxl_hip.so's HIP kernels.
"""
import ctypes as C

import torch

from . import abi


def _check(L, ctx, rc, what):
    if rc != 0:
        msg = L.jxlhip_last_error(ctx) if ctx else b""
        raise abi.JxlHipError(
            f"{what}: {L.jxlhip_status_string(rc).decode()} ({rc}) {msg.decode() if msg else ''}")


class VarDctDecoder:
    """One decoder context bound to one GPU (one per process / rank)."""

    def __init__(self, device=0, use_torch_stream=True):
        self.L = abi.load_library()
        self.device = int(device)
        if not torch.cuda.is_available():
            raise abi.JxlHipError("no HIP device visible: the VarDCT back-end has no CPU path")
        self.ctx = C.c_void_p()
        _check(self.L, None, self.L.jxlhip_create(self.device, C.byref(self.ctx)), "jxlhip_create")
        if use_torch_stream:
            s = torch.cuda.current_stream(self.device).cuda_stream
            _check(self.L, self.ctx, self.L.jxlhip_set_stream(self.ctx, C.c_void_p(s), 1), "set_stream")
        self.params = None
        self._keep = None
        self.out = None
        self.out_size = None
        self._ref_sizes = {}  # set_reference_frame: slot -> (xsize, ysize)

    def close(self):
        if self.ctx:
            self.L.jxlhip_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- frame set-up ------------------------------------------------------
    def begin_frame(self, params):
        """params: abi.FrameParams (or dict from synth.synth_frame)."""
        if isinstance(params, dict):
            params = abi.make_params(params)
        self.params = params
        self.out_size = None  # (xsize, ysize) of an upsampled frame's output: set_upsampling
        self.image_size = None  # (xsize, ysize) of the image a blended frame is written at: set_blending
        _check(self.L, self.ctx, self.L.jxlhip_frame_begin(self.ctx, C.byref(params)), "frame_begin")

    def default_dequant_tables(self):
        t = torch.empty(2056 * 64 * 3, dtype=torch.float32, device=f"cuda:{self.device}")
        _check(self.L, self.ctx, self.L.jxlhip_default_dequant_tables(self.ctx, C.c_void_p(t.data_ptr())), "default_dequant_tables")
        return t

    def dequant_tables(self, encodings=None):
        """The 17 dequant tables of abi.QuantEncodings (None = the default library)."""
        t = torch.empty(2056 * 64 * 3, dtype=torch.float32, device=f"cuda:{self.device}")
        e = None if encodings is None else C.cast(C.byref(encodings), C.c_void_p)
        _check(self.L, self.ctx, self.L.jxlhip_dequant_tables(self.ctx, e, C.c_void_p(t.data_ptr())), "dequant_tables")
        return t

    def set_inputs(self, tensors, dequant_table):
        """tensors: dict of CUDA tensors laid out as jxlhip_frame_inputs."""
        dev = f"cuda:{self.device}"
        for k, v in tensors.items():
            for t in (v if isinstance(v, (list, tuple)) else [v]):
                assert t.is_cuda and t.is_contiguous(), k
        fi = abi.FrameInputs()
        for c in range(3):
            fi.coeffs[c] = tensors["coeffs"][c].data_ptr()
            fi.dc[c] = tensors["dc"][c].data_ptr()
        fi.ac_strategy = tensors["ac_strategy"].data_ptr()
        fi.raw_quant = tensors["raw_quant"].data_ptr()
        fi.epf_sharpness = tensors["epf_sharpness"].data_ptr()
        fi.ytox_map = tensors["ytox_map"].data_ptr()
        fi.ytob_map = tensors["ytob_map"].data_ptr()
        fi.dequant_table = dequant_table.data_ptr()
        self._keep = (tensors, dequant_table, dev)
        _check(self.L, self.ctx, self.L.jxlhip_frame_set_inputs(self.ctx, C.byref(fi)), "frame_set_inputs")

    # -- geometry ------------------------------------------------------------
    def stripe_rows(self):
        p = self.params
        ysg = (p.ysize + 255) // 256
        g0 = p.stripe_group_y0
        gr = p.stripe_group_rows if p.stripe_group_rows else ysg - g0
        y0 = g0 * 256
        y1 = min(p.ysize, (g0 + gr) * 256)
        return y0, y1

    def alloc_output(self):
        p = self.params
        y0, y1 = self.stripe_rows()
        dev = f"cuda:{self.device}"
        # undo_orientation 5..8: the display frame is ysize pixels wide and xsize rows high
        oh, ow = (p.xsize, p.ysize) if p.undo_orientation >= 5 else (y1 - y0, p.xsize)
        if self.out_size is not None:  # an upsampled frame (whole frames, coded orientation)
            ow, oh = self.out_size
        if self.image_size is not None:  # a blended frame: the caller's buffer is the image
            ow, oh = self.image_size
        if p.output_kind == 1:
            return torch.empty((oh, ow, 3), dtype=torch.float32, device=dev)
        if p.output_kind == 2:  # packed RGB(A): dtype of the sample type (F16 as raw uint16 bits)
            dt = {0: torch.float32, 1: torch.uint8, 2: torch.int16, 3: torch.int16}[p.out_format.sample_type]
            return torch.empty((oh, ow, p.out_format.num_channels), dtype=dt, device=dev)
        if self.out_size is not None:
            return torch.empty((3, oh, ow), dtype=torch.float32, device=dev)
        return torch.empty((3, y1 - y0, p.xsize), dtype=torch.float32, device=dev)

    def _out_args(self, out):
        p = self.params
        if p.output_kind == 1:
            return C.c_void_p(out.data_ptr()), out.stride(0) * 4, 0
        if p.output_kind == 2:
            return C.c_void_p(out.data_ptr()), out.stride(0) * out.element_size(), 0
        return C.c_void_p(out.data_ptr()), out.stride(1), out.stride(0)

    def set_alpha(self, plane):
        """The frame's alpha channel for 4-channel packed outputs: a host float32 array [ysize, xsize] (1.0 = opaque),
        jxlhip_set_alpha; begin_frame resets to opaque."""
        import numpy as np
        a = np.ascontiguousarray(plane, dtype=np.float32)
        assert a.shape == (self.params.ysize, self.params.xsize), a.shape
        _check(self.L, self.ctx, self.L.jxlhip_set_alpha(self.ctx, a.ctypes.data, a.shape[1]), "set_alpha")
        self.sync()  # (the array may go away as soon as this returns)

    def set_noise(self, lut, visible_frame_index=1, nonvisible_frame_index=0):
        """Photon noise of the current frame (FrameHeader::kNoise): NoiseParams::lut (8 floats) and the generators'
        seed indices (a file's only frame: 1, 0), jxlhip_set_noise; begin_frame resets to no noise."""
        vals = [float(v) for v in lut]
        assert len(vals) == 8, len(vals)
        _check(self.L, self.ctx, self.L.jxlhip_set_noise(self.ctx, (C.c_float * 8)(*vals), int(visible_frame_index),
                                                         int(nonvisible_frame_index)), "set_noise")

    def set_splines(self, splines, quantization_adjustment=0):
        """Splines of the current frame (FrameHeader::kSplines), jxlhip_set_splines: a jxlhip_splines* handle
        (abi.splines_from_quantized, jxlhip_splines_decode) or a list of quantized splines in the form
        abi.splines_from_quantized takes; None = no splines.  begin_frame resets to no splines."""
        if splines is None or isinstance(splines, (int, C.c_void_p)):
            _check(self.L, self.ctx, self.L.jxlhip_set_splines(self.ctx, splines), "set_splines")
            return
        rc, h = abi.splines_from_quantized(splines, quantization_adjustment, self.L)
        _check(self.L, self.ctx, rc, "splines_from_quantized")
        try:
            _check(self.L, self.ctx, self.L.jxlhip_set_splines(self.ctx, h), "set_splines")
        finally:
            abi.splines_destroy(h, self.L)

    def set_reference_frame(self, slot, planes):
        """A reference frame for patches, jxlhip_set_reference_frame: planes = float32 XYB of shape [3, ysize, xsize]
        (a host array, or a CUDA tensor of this device) into slot 0..3 of the context; None clears the slot.  The slots
        outlive frames."""
        import numpy as np
        if planes is None:
            _check(self.L, self.ctx, self.L.jxlhip_set_reference_frame(self.ctx, int(slot), 0, 0, (C.c_void_p * 3)(), 0, 0),
                   "set_reference_frame")
            self._ref_sizes.pop(int(slot), None)
            return
        on_device = isinstance(planes, torch.Tensor) and planes.is_cuda
        if on_device:
            a = planes.to(torch.float32).contiguous()
            base, esz = a.data_ptr(), 4
        else:
            a = np.ascontiguousarray(planes, dtype=np.float32)
            base, esz = a.ctypes.data, 4
        assert a.ndim == 3 and a.shape[0] == 3, tuple(a.shape)
        h, w = int(a.shape[1]), int(a.shape[2])
        ptrs = (C.c_void_p * 3)(*[base + k * h * w * esz for k in range(3)])
        _check(self.L, self.ctx, self.L.jxlhip_set_reference_frame(self.ctx, int(slot), w, h, ptrs, w, int(on_device)),
               "set_reference_frame")  # (synchronous: `a` may go away)
        self._ref_sizes[int(slot)] = (w, h)

    def set_patches(self, patches):
        """Patches of the current frame (FrameHeader::kPatches), jxlhip_set_patches: a jxlhip_patches* handle
        (abi.patches_from_list, abi.patches_decode) or a list of patch dicts in the form abi.patches_from_list takes,
        checked against the slots set_reference_frame has filled; None = no patches.  begin_frame resets to no patches."""
        if patches is None or isinstance(patches, (int, C.c_void_p)):
            _check(self.L, self.ctx, self.L.jxlhip_set_patches(self.ctx, patches), "set_patches")
            return
        p = self.params
        rc, h = abi.patches_from_list(patches, (p.xsize + 7) & ~7, (p.ysize + 7) & ~7, self._ref_sizes, L=self.L)
        _check(self.L, self.ctx, rc, "patches_from_list")
        try:
            _check(self.L, self.ctx, self.L.jxlhip_set_patches(self.ctx, h), "set_patches")
        finally:
            abi.patches_destroy(h, self.L)

    def set_upsampling(self, factor, out_size, weights=None):
        """Upsampling of the current frame (FrameHeader::upsampling: 2, 4 or 8), jxlhip_set_upsampling: begin_frame's
        size is the coded size, out_size = (xsize, ysize) the image the frame is upsampled and cropped to; weights =
        the factor's 15 / 55 / 210 coded weights, None = the format's defaults.  Call it before set_splines.
        decode_frame() then allocates the output-sized tensor.  factor 1 or begin_frame resets."""
        w = None
        if weights is not None:
            vals = [float(v) for v in weights]
            assert len(vals) == {2: 15, 4: 55, 8: 210}[int(factor)], len(vals)
            w = (C.c_float * len(vals))(*vals)
        ox, oy = (int(out_size[0]), int(out_size[1])) if out_size is not None else (0, 0)
        _check(self.L, self.ctx, self.L.jxlhip_set_upsampling(self.ctx, int(factor), w, ox, oy), "set_upsampling")
        self.out_size = (ox, oy) if int(factor) > 1 else None

    def set_dc_only_groups(self, mask, weights=None):
        """The AC groups of the current frame that have no AC and are drawn from their DC upsampled 8x,
        jxlhip_set_dc_only_groups: mask = one truth value per group (row-major over the frame's 256 x 256 groups),
        weights = the 210 coded weights of the 8x upsampler, None = the format's defaults.  None or an all-zero mask
        leaves the frame on its own path; begin_frame resets."""
        import numpy as np
        p = self.params
        ng = ((p.xsize + 255) // 256) * ((p.ysize + 255) // 256)
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
            assert m.size == ng, (m.size, ng)
        w = None
        if weights is not None:
            vals = [float(v) for v in weights]
            assert len(vals) == 210, len(vals)
            w = (C.c_float * 210)(*vals)
        _check(self.L, self.ctx, self.L.jxlhip_set_dc_only_groups(self.ctx, m.ctypes.data if m is not None else None, w),
               "set_dc_only_groups")

    def set_blending(self, image_size, origin=(0, 0), mode=abi.BLEND_REPLACE, clamp=False, source=0, save_slot=None):
        """Blending of the current frame, jxlhip_set_blending: the frame's own output is blended at `origin` = (x0, y0)
        (signed) over the canvas of slot `source` with BlendMode `mode` (abi.BLEND_*), written at image_size =
        (xsize, ysize) and saved into save_slot (0..3; None = not saved).  decode_frame() then allocates an
        image-sized tensor; decode_frame(out=False) only saves.  None instead of image_size switches blending off;
        begin_frame resets."""
        if image_size is None:
            _check(self.L, self.ctx, self.L.jxlhip_set_blending(self.ctx, None), "set_blending")
            self.image_size = None
            return
        b = abi.BlendParams(int(image_size[0]), int(image_size[1]), int(origin[0]), int(origin[1]), int(mode), int(bool(clamp)),
                            int(source), abi.BLEND_NO_SAVE if save_slot is None else int(save_slot))
        _check(self.L, self.ctx, self.L.jxlhip_set_blending(self.ctx, C.byref(b)), "set_blending")
        self.image_size = (b.image_xsize, b.image_ysize)

    def set_blending_extra(self, planes, channels, color_alpha_channel=0):
        """The extra channels of the current blended frame, jxlhip_set_blending_extra (after set_blending): planes =
        float32 host array [n, ysize, xsize] at the frame's own size, channels = one dict per channel with is_alpha,
        alpha_associated, mode (abi.BLEND_*), alpha_channel, clamp, source (each defaults to 0), color_alpha_channel =
        the alpha channel of the colour's kBlend / kAlphaWeightedAdd.  begin_frame and set_blending reset it."""
        import numpy as np
        a = np.ascontiguousarray(planes, dtype=np.float32)
        assert a.ndim == 3 and a.shape[0] == len(channels) and 1 <= len(channels) <= 4, (tuple(a.shape), len(channels))
        e = abi.BlendExtraParams()
        e.num_extra_channels = len(channels)
        e.color_alpha_channel = int(color_alpha_channel)
        e.stride_floats = int(a.shape[2])
        for i, ch in enumerate(channels):
            for k in ("is_alpha", "alpha_associated", "mode", "alpha_channel", "clamp", "source"):
                setattr(e.channel[i], k, int(ch.get(k, 0)))
            e.planes[i] = a[i].ctypes.data
        _check(self.L, self.ctx, self.L.jxlhip_set_blending_extra(self.ctx, C.byref(e)), "set_blending_extra")
        self.sync()  # (`a` may go away)

    def set_tone_mapping(self, orig_nits, desired_nits=None, luminances=(0.2126, 0.7152, 0.0722), orig_transfer=abi.TF_PQ):
        """Tone mapping of the current frame, jxlhip_set_tone_mapping: an original mastered at orig_nits (transfer
        function orig_transfer, abi.TF_*) shown on a display of desired_nits, luminances = those of the OUTPUT
        primaries.  Call it after begin_frame, which resets it; None instead of orig_nits switches it off.  A display at
        least as bright as the original leaves the frame on its plain path."""
        if orig_nits is None:
            _check(self.L, self.ctx, self.L.jxlhip_set_tone_mapping(self.ctx, None), "set_tone_mapping")
            return
        t = abi.ToneMapping(float(orig_nits), float(desired_nits), (C.c_float * 3)(*[float(v) for v in luminances]),
                            int(orig_transfer))
        _check(self.L, self.ctx, self.L.jxlhip_set_tone_mapping(self.ctx, C.byref(t)), "set_tone_mapping")

    def set_display(self, display_nits=0.0, primaries=None, white_point=None):
        """The display the whole-file decode calls render for, jxlhip_codestream_set_display (sticky on the context):
        display_nits = its peak luminance (0: no tone mapping), primaries = "srgb" | "p3" | "rec2100" | abi.PRIM_* |
        None (the original's), white_point = abi.WP_* | None (D65 when primaries are named, else the original's).
        set_display() with nothing resets."""
        prim = {None: 0, "srgb": abi.PRIM_SRGB, "p3": abi.PRIM_P3, "rec2100": abi.PRIM_2100}.get(primaries, primaries)
        wp = int(white_point) if white_point else (abi.WP_D65 if prim else 0)
        if not display_nits and not prim and not wp:
            _check(self.L, self.ctx, self.L.jxlhip_codestream_set_display(self.ctx, None), "set_display")
            return
        d = abi.Display(float(display_nits), int(prim), wp)
        _check(self.L, self.ctx, self.L.jxlhip_codestream_set_display(self.ctx, C.byref(d)), "set_display")

    def read_canvas(self, slot):
        """The canvas of slot 0..3 (a frame saved by set_blending's save_slot) as a float32 CUDA tensor [ysize, xsize, 3]
        in the transfer function of the frames that made it; None when the slot holds no canvas."""
        w, h = C.c_uint32(), C.c_uint32()
        _check(self.L, self.ctx, self.L.jxlhip_canvas_read(self.ctx, int(slot), None, 0, C.byref(w), C.byref(h)), "canvas_read")
        if w.value == 0:
            return None
        t = torch.empty((h.value, w.value, 3), dtype=torch.float32, device=f"cuda:{self.device}")
        _check(self.L, self.ctx, self.L.jxlhip_canvas_read(self.ctx, int(slot), C.c_void_p(t.data_ptr()), 3 * w.value,
                                                          C.byref(w), C.byref(h)), "canvas_read")
        self.sync()
        return t

    def read_canvas_extra(self, slot, ec):
        """Plane `ec` of the canvas of slot 0..3 (jxlhip_canvas_read_extra) as a float32 CUDA tensor [ysize, xsize]; None
        when the slot holds no canvas or its canvas no such plane."""
        w, h = C.c_uint32(), C.c_uint32()
        _check(self.L, self.ctx, self.L.jxlhip_canvas_read_extra(self.ctx, int(slot), int(ec), None, 0, C.byref(w), C.byref(h)),
               "canvas_read_extra")
        if w.value == 0:
            return None
        t = torch.empty((h.value, w.value), dtype=torch.float32, device=f"cuda:{self.device}")
        _check(self.L, self.ctx, self.L.jxlhip_canvas_read_extra(self.ctx, int(slot), int(ec), C.c_void_p(t.data_ptr()), w.value,
                                                                C.byref(w), C.byref(h)), "canvas_read_extra")
        self.sync()
        return t

    def read_frame_extra(self, ec):
        """The blended plane of extra channel `ec` of the frame just decoded with set_blending_extra
        (jxlhip_frame_extra_read), at image size, as a float32 CUDA tensor [ysize, xsize]."""
        w, h = self.image_size
        t = torch.empty((h, w), dtype=torch.float32, device=f"cuda:{self.device}")
        _check(self.L, self.ctx, self.L.jxlhip_frame_extra_read(self.ctx, int(ec), C.c_void_p(t.data_ptr()), w), "frame_extra_read")
        self.sync()
        return t

    # -- decode ----------------------------------------------------------------
    def decode_blocks(self):
        _check(self.L, self.ctx, self.L.jxlhip_decode_blocks(self.ctx), "decode_blocks")

    def decode_filters(self, out, rows=None):
        """Phase 2 into `out` (the stripe's rows).  rows = (y_begin, y_end): only those frame rows (block-row multiples
        inside the stripe, jxlhip_decode_filters_rows) -- the interior first while the halo rows travel."""
        a = self._out_args(out)
        if rows is None:
            _check(self.L, self.ctx, self.L.jxlhip_decode_filters(self.ctx, *a), "decode_filters")
        else:
            _check(self.L, self.ctx, self.L.jxlhip_decode_filters_rows(self.ctx, *a, int(rows[0]), int(rows[1])), "decode_filters_rows")

    def decode_frame(self, out=None):
        if out is False:  # a blended frame that is only saved (set_blending with a save_slot)
            _check(self.L, self.ctx, self.L.jxlhip_decode_frame(self.ctx, None, 0, 0), "decode_frame")
            return None
        if out is None:
            out = self.alloc_output()
        a = self._out_args(out)
        _check(self.L, self.ctx, self.L.jxlhip_decode_frame(self.ctx, *a), "decode_frame")
        return out

    def sync(self):
        _check(self.L, self.ctx, self.L.jxlhip_sync(self.ctx), "sync")

    # -- taps / profiling --------------------------------------------------------
    def export_xyb(self):
        """Row-major copies of the phase-1 XYB planes (the stripe's block-padded
        rows x padded width), as numpy arrays."""
        p = self.params
        xsb = (p.xsize + 7) // 8
        y0, y1 = self.stripe_rows()
        rows = (y1 - y0 + 7) // 8 * 8
        outs = [torch.empty((rows, xsb * 8), dtype=torch.float32, device=f"cuda:{self.device}")
                for _ in range(3)]
        ptrs = (C.c_void_p * 3)(*[o.data_ptr() for o in outs])
        _check(self.L, self.ctx, self.L.jxlhip_export_xyb(self.ctx, ptrs, xsb * 8), "export_xyb")
        self.sync()
        return [o.cpu().numpy() for o in outs]

    def sigma(self):
        ptr, stride = C.c_void_p(), C.c_size_t()
        _check(self.L, self.ctx, self.L.jxlhip_get_sigma(self.ctx, C.byref(ptr), C.byref(stride)), "get_sigma")
        p = self.params
        ysb = (p.ysize + 7) // 8
        return _as_tensor(ptr.value, ysb * stride.value, torch.float32, self.device).reshape(ysb, stride.value).clone()

    def halo_rows(self):
        return self.L.jxlhip_halo_rows(self.ctx)

    def halo_export(self, which, buf=None):
        """Dense [3, halo, xsize] tensor with this stripe's first (which=0) or
        last (which=1) halo rows (written into `buf` when given)."""
        p = self.params
        if buf is None:
            buf = torch.empty((3, self.halo_rows(), p.xsize), dtype=torch.float32,
                              device=f"cuda:{self.device}")
        _check(self.L, self.ctx, self.L.jxlhip_halo_export(self.ctx, which, C.c_void_p(buf.data_ptr())), "halo_export")
        return buf

    def halo_import(self, which, buf):
        """Installs rows received from the stripe above (which=0) / below (1)."""
        assert buf.is_cuda and buf.is_contiguous() and buf.dtype == torch.float32
        assert tuple(buf.shape) == (3, self.halo_rows(), self.params.xsize)
        _check(self.L, self.ctx, self.L.jxlhip_halo_import(self.ctx, which, C.c_void_p(buf.data_ptr())), "halo_import")

    def set_stream(self, stream):
        """All launches of this context go to `stream` (a torch.cuda.Stream) from now on."""
        _check(self.L, self.ctx, self.L.jxlhip_set_stream(self.ctx, C.c_void_p(stream.cuda_stream), 1), "set_stream")

    def stripe_begin(self, send_up=None, send_down=None):
        """Phase 1 of the stripe + its boundary rows into the dense [3, halo, xsize] send buffers (None = no neighbour
        on that side): one call (jxlhip_stripe_begin)."""
        a = C.c_void_p(send_up.data_ptr()) if send_up is not None else None
        b = C.c_void_p(send_down.data_ptr()) if send_down is not None else None
        _check(self.L, self.ctx, self.L.jxlhip_stripe_begin(self.ctx, a, b), "stripe_begin")

    def stripe_finish(self, out, recv_up=None, recv_down=None, interior=None):
        """The neighbours' rows installed + phase 2 of every row outside interior = (y_begin, y_end), which
        decode_filters(rows=interior) has filtered already (None: of every row): one call (jxlhip_stripe_finish)."""
        a = C.c_void_p(recv_up.data_ptr()) if recv_up is not None else None
        b = C.c_void_p(recv_down.data_ptr()) if recv_down is not None else None
        ya, yb = (int(interior[0]), int(interior[1])) if interior else (0, 0)
        _check(self.L, self.ctx, self.L.jxlhip_stripe_finish(self.ctx, a, b, *self._out_args(out), ya, yb), "stripe_finish")

    def set_concurrency_hint(self, frames_in_flight):
        """How many contexts the caller keeps busy on this device at a time (a pool of decoders): moves the frame size
        from which decode_frame takes the fused kernel (12 Mpx alone, 6 Mpx with several frames in flight)."""
        _check(self.L, self.ctx, self.L.jxlhip_set_concurrency_hint(self.ctx, int(frames_in_flight)), "set_concurrency_hint")

    def prepare_launches(self):
        """(launched, reused): k_prepare launches this context has enqueued and decode calls that saved one by reusing
        an earlier decode's work lists (jxlhip_debug_prepare_launches; direct calls only)."""
        a, b = C.c_uint64(), C.c_uint64()
        _check(self.L, self.ctx, self.L.jxlhip_debug_prepare_launches(self.ctx, C.byref(a), C.byref(b)), "prepare_launches")
        return a.value, b.value

    def profile(self, enable=True):
        _check(self.L, self.ctx, self.L.jxlhip_profile_enable(self.ctx, int(enable)), "profile_enable")

    def profile_read(self):
        ms = (C.c_float * abi.KERNEL_COUNT_EX)()
        n = (C.c_uint32 * abi.KERNEL_COUNT_EX)()
        _check(self.L, self.ctx, self.L.jxlhip_profile_read_ex(self.ctx, ms, n, abi.KERNEL_COUNT_EX), "profile_read")
        return {abi.KERNEL_NAMES_EX[i]: (ms[i], n[i]) for i in range(abi.KERNEL_COUNT_EX) if n[i]}


class _CudaArray:
    """Minimal __cuda_array_interface__ holder for zero-copy torch views of
    context-owned HBM."""

    def __init__(self, ptr, nelem, typestr):
        self.__cuda_array_interface__ = {
            "shape": (nelem,), "typestr": typestr, "data": (int(ptr), False),
            "version": 2, "strides": None}


def _as_tensor(ptr, nelem, dtype, device):
    assert dtype == torch.float32
    return torch.as_tensor(_CudaArray(ptr, nelem, "<f4"), device=f"cuda:{device}")
