"""Random sequences of C-ABI calls that also move and edit the scene, trace rays and paths, render guides, denoise, reproject
and display, against the model of api_fuzz_cases.py (GPU).

ptmi_set_camera, ptmi_set_camera_reprojected, ptmi_update_triangles(_device), ptmi_update_materials, ptmi_update_lights,
ptmi_set_sky, refused updates, edits and cameras, ptmi_query_rays(_device), ptmi_trace_paths(_device),
ptmi_render_guides(_device), ptmi_denoise(_device), ptmi_read_display_tonemapped, ptmi_display_device and
ptmi_luminance_histogram(_device) between renders, snapshots, bursts, reads, clears and re-uploads, and between the calls of a walk, while
launches for calls that have not been made yet are in flight - on one device and on one device listed two or three times, at
the default launch size and at caps of 1 to 3 iterations per launch.  What ptmi_query.cpp, ptmi_guides.cpp and ptmi_denoise.cpp
promise in prose (they touch nothing but their planes; the calls that rewrite scene records wait for their stream first; the
filter reads the image ptmi_read_image would return) is what the model assumes.  One device: bit for bit.  Several: sample
counts, histograms and counters exactly, colour sums up to their association.  Hits and guide planes: bit for bit on any device
count (both run on devices[0] alone).  Filtered images: every word equal to denoise_cases.denoise of the image and the guide
planes the context returns, which are themselves held against the model, on any device count; through device pointers, of the
guide planes read back and the model's accumulators at the call (one device) or planes of the caller's.  Path sums: every word
equal to path_query_cases.Yardstick on the scene as updated and edited so far, on any device count.  A reprojected camera: the
next read against reproject_cases.reproject of the model's accumulators, as any other read (one device: bit for bit).
Displayed pixels and luminance histograms: every byte and word equal to display_cases.py of the image the context returns
(held against the model), of the model's accumulators at the call, of planes of the caller's, or of the tensor the denoise call
just before has written.  This is the one test that holds a render after ptmi_update_materials / ptmi_update_lights /
ptmi_set_sky against the CPU oracle; test_scene_edit_gpu.py holds it against a second context.  The scripts, their coverage
and the model are checked without a GPU in test_api_fuzz_model.py."""
import os

import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, backend, structs as S
import api_fuzz_cases as F
import gpu_cases
import guide_cases as G
import path_query_cases as P

pytestmark = pytest.mark.gpu


class DeviceIO:
    """ptmi_query_rays_device / ptmi_render_guides_device / ptmi_denoise_device / ptmi_trace_paths_device / ptmi_display_device /
    ptmi_luminance_histogram_device on torch tensors on device 0.  No call is waited for: the result is collected (after
    ptmi_synchronize) when the executor asks, one operation later; the tensors live until then.  ptmi_update_triangles_device
    is synchronous."""

    def query(self, be, rays, any_hit):
        import torch
        d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(len(rays), 12).copy()).cuda()
        d_hits = torch.full((len(rays), 12), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        be.query_rays_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), any_hit=any_hit)

        def collect(keep=d_rays):  # (the rays stay allocated until the hits are read)
            be.synchronize()
            return np.ascontiguousarray(d_hits.cpu().numpy()).view(S.RAY_HIT).reshape(-1)

        return collect

    def guides(self, be, first, n, planes):
        import torch
        tensors = {name: torch.full((F.H, F.W) if name == "hit_count" else (F.H, F.W, 4), -1, dtype=torch.int32 if name == "ids" else torch.float32,
                                    device="cuda") for name in G.PLANES}
        torch.cuda.synchronize()
        be.render_guides_device(first, n, **{name: tensors[name].data_ptr() for name in planes})

        def collect():
            be.synchronize()
            got = {name: (t.cpu().numpy().view(np.uint32) if name == "ids" else t.cpu().numpy()) for name, t in tensors.items()}
            for name in G.PLANES:  # a plane that is not asked for is not written
                if name not in planes:
                    assert (got[name] == (0xFFFFFFFF if name == "ids" else -1.0)).all(), f"guides wrote the plane {name}, which was not asked for"
            return {name: got[name] for name in planes}

        return collect

    def denoise(self, be, first, n, image, params):
        """ptmi_render_guides_device into four tensors, then ptmi_denoise_device guided by them: on the context's own accumulators
        (image None) or on the caller's (colour sums, counts).  Collected: (the result, the four guide planes as they are read
        back); the image planes must come back as they were sent, and the result tensor starts as -1 everywhere."""
        import torch
        guides = {name: torch.full((F.H, F.W) if name == "hit_count" else (F.H, F.W, 4), -1.0, dtype=torch.float32, device="cuda")
                  for name in F.DENOISE_PLANES}
        out = torch.full((F.H, F.W, 4), -1.0, dtype=torch.float32, device="cuda")
        sent = [] if image is None else [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in image]
        torch.cuda.synchronize()
        be.render_guides_device(first, n, **{name: t.data_ptr() for name, t in guides.items()})
        be.denoise_device(out.data_ptr(), {name: t.data_ptr() for name, t in guides.items()}, *(t.data_ptr() for t in sent), **params)
        self.denoised = out  # (what a display call made next shows: the viewer's pipeline)

        def collect():
            be.synchronize()
            for t, a in zip(sent, image or ()):
                assert np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32)), "denoise wrote an image plane of the caller's"
            return out.cpu().numpy(), {name: t.cpu().numpy() for name, t in guides.items()}

        return collect

    def update(self, be, tris):
        """ptmi_update_triangles_device from a 16-byte-aligned float32 (n, 84) tensor (a byte copy of the records).  Synchronous."""
        t = gpu_cases.tensor_on_device(np.frombuffer(bytearray(np.ascontiguousarray(tris).tobytes()), np.float32).reshape(len(tris), 84))
        assert t.data_ptr() % 16 == 0
        return be.update_triangles_device(t.data_ptr(), len(tris))

    def paths(self, be, rays, first_iteration, n_iterations, first_index):
        import torch
        d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(len(rays), 12).copy()).cuda()
        d_sums = torch.full((len(rays), 12), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        be.trace_paths_device(d_rays.data_ptr(), len(rays), d_sums.data_ptr(), first_iteration, n_iterations, first_index, P.STRIDE)

        def collect(keep=d_rays):  # (the rays stay allocated until the sums are read)
            be.synchronize()
            return np.ascontiguousarray(d_sums.cpu().numpy()).view(S.PATH_SUM).reshape(-1)

        return collect

    def _planes(self, image):
        """The device planes of a display call, and what was sent: none (the context's own accumulators), sums and counts, or
        a mean plane alone - a seeded one, or the tensor the denoise call made just before wrote."""
        import torch
        if image is None:
            return [], []
        if isinstance(image[0], str) and image[0] == "denoised":
            return [self.denoised], []
        sent = [image[1]] if isinstance(image[0], str) else list(image)
        return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in sent], sent

    @staticmethod
    def _unwritten(planes, sent, who):
        for t, a in zip(planes, sent):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32)), f"{who} wrote an image plane of the caller's"

    def display(self, be, image, params):
        """ptmi_display_device.  Collected: (the pixels, the mean plane as it is read back or None)"""
        import torch
        planes, sent = self._planes(image)
        shape = (F.H, F.W, 4) if params["rgba"] else (F.H, (3 * F.W + 3) & ~3)
        out = torch.full(shape, 0xAA, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        be.display_device(out.data_ptr(), *(t.data_ptr() for t in planes), **params)

        def collect():
            be.synchronize()
            self._unwritten(planes, sent, "display")
            return out.cpu().numpy(), (planes[0].cpu().numpy() if len(planes) == 1 else None)

        return collect

    def histogram(self, be, image):
        """ptmi_luminance_histogram_device into 260 words of garbage, which the call zeroes on the stream"""
        import torch
        planes, sent = self._planes(image)
        out = torch.full((backend.LUMINANCE_WORDS,), -559038737, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        be.luminance_histogram_device(out.data_ptr(), *(t.data_ptr() for t in planes))

        def collect():
            be.synchronize()
            self._unwritten(planes, sent, "histogram")
            return out.cpu().numpy().view(np.uint32), (planes[0].cpu().numpy() if len(planes) == 1 else None)

        return collect


def play(seed, cap, devices, super_sampling=False):
    da, megakernel = F.flags_of(seed, super_sampling)
    flags = (backend.FLAG_DEFAULT_ARITHMETIC if da else 0) | (backend.FLAG_MEGAKERNEL if megakernel else 0)
    ops = F.script(seed, devices, cap, super_sampling)
    lights = F.WORLD.anchor(ops[0][1]).lightsSize
    assert all(F.WORLD.anchor(name).lightsSize == lights for name in F.SCENES)  # (one context takes them all)
    be = Backend().setup_context(F.W, F.H, F.D, lights, S.JITTERED, super_sampling=super_sampling, flags=flags, devices=devices)
    try:
        return F.run(ops, be, F.Model(F.WORLD, da, super_sampling), io=DeviceIO(), exact=devices is None)
    finally:
        be.release()


@pytest.mark.parametrize("devices", list(F.DEVICES))
@pytest.mark.parametrize("seed, cap", [pytest.param(seed, None, id=str(seed)) for seed in range(int(os.environ.get("PTMI_API_FUZZ_SEEDS", F.DEFAULT_SEEDS)))] +
                         [pytest.param(seed, cap, id=f"{seed}-cap{cap}") for seed, cap in F.LOW_CAP_SEEDS])  # (a soak: PTMI_API_FUZZ_SEEDS=400)
def test_random_scene_call_sequences(seed, cap, devices, monkeypatch):
    if cap is not None:
        monkeypatch.setenv("PTMI_ITERATIONS_PER_LAUNCH", str(cap))
    made = play(seed, cap, F.DEVICES[devices])
    print("operations made:", dict(sorted(made.items())))


@pytest.mark.parametrize("seed", F.SUPER_SAMPLING_SEEDS)
def test_random_scene_call_sequences_super_sampling(seed):
    """The same for an adaptive (SUPER_SAMPLING) context, whose every iteration depends on the accumulators and the variance image
    it finds: the model is the oracle run statefully on the yardstick scene of the state each render was made in.  Bit for bit,
    the variance image included."""
    made = play(seed, None, None, super_sampling=True)
    print("operations made:", dict(sorted(made.items())))
