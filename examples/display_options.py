"""What examples/denoise.py and examples/orbit.py share: the --tone / --transfer / --exposure options, and the denoised image
brought down as displayed pixels - guides, filter and display run between device tensors, so 3 bytes per pixel cross the bus and
no float plane does."""
import opencl_pathtracer_amd as pt

TONES = dict(clamp=pt.backend.TONE_CLAMP, reinhard=pt.backend.TONE_REINHARD, filmic=pt.backend.TONE_FILMIC)
TRANSFERS = dict(linear=pt.backend.TRANSFER_LINEAR, srgb=pt.backend.TRANSFER_SRGB, gamma22=pt.backend.TRANSFER_GAMMA22)


def add_arguments(ap):
    ap.add_argument("--tone", choices=sorted(TONES), help="display on the device (ptmi_display_device) with this tone operator")
    ap.add_argument("--transfer", choices=sorted(TRANSFERS), help="... and this display transfer function")
    ap.add_argument("--exposure", help="... and this exposure: a number, or `auto` (middle grey from the luminance histogram)")


def chosen(args):
    """None without any of the three options (the reference viewer's linear clamp, quantised on the host, as before), else the
    tone and transfer keywords of Backend.display; what was not given is the shipped default.  Call it before the first context
    is set up: torch's HIP runtime has to find the device before the library's does."""
    if args.tone is None and args.transfer is None and args.exposure is None:
        return None
    import torch
    torch.cuda.init()
    d = pt.backend.DISPLAY_DEFAULTS
    return dict(tone=d["tone"] if args.tone is None else TONES[args.tone],
                transfer=d["transfer"] if args.transfer is None else TRANSFERS[args.transfer])


def exposure_of(be, args):
    """--exposure as a number; `auto`: from the histogram of the context's image, counted on the device (1040 bytes come down)"""
    if args.exposure is None:
        return pt.backend.DISPLAY_DEFAULTS["exposure"]
    if args.exposure == "auto":
        return pt.backend.exposure_from_histogram(be.luminance_histogram())
    return float(args.exposure)


def denoised_rows(be, exposure, display, **denoise):
    """B,G,R scanlines of the denoised image: render_guides_device -> denoise_device -> display_device on tensors, one copy of
    H * stride bytes to the host.  `denoise`: the keywords of Backend.denoise_device, guide_first_iteration and guide_iterations
    among them."""
    import torch
    h, w, device = be.cfg.image_height, be.cfg.image_width, torch.device("cuda", be.cfg.device)
    planes = {name: torch.empty((h, w) if name == "hit_count" else (h, w, 4), dtype=torch.float32, device=device)
              for name in ("albedo", "normal", "position", "hit_count")}
    mean = torch.empty((h, w, 4), dtype=torch.float32, device=device)
    rows = torch.empty((h, (3 * w + 3) & ~3), dtype=torch.uint8, device=device)
    torch.cuda.synchronize(device)  # (the context's stream is not torch's)
    pointers = {name: t.data_ptr() for name, t in planes.items()}
    be.render_guides_device(denoise["guide_first_iteration"], denoise["guide_iterations"], **pointers)
    be.denoise_device(mean.data_ptr(), pointers, **denoise)
    be.display_device(rows.data_ptr(), mean.data_ptr(), exposure=exposure, **display)  # (a mean plane: no counts)
    be.synchronize()
    return rows.cpu().numpy()
