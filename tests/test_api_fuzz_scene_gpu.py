"""Random sequences of C-ABI calls that also move the scene, trace rays, render guides and denoise, against the model of
api_fuzz_cases.py (GPU).

ptmi_set_camera, ptmi_update_triangles, refused updates and cameras, ptmi_query_rays(_device), ptmi_render_guides(_device) and
ptmi_denoise(_device) between renders, snapshots, bursts, reads, clears and re-uploads, and between the calls of a walk, while
launches for calls that have not been made yet are in flight - on one device and on one device listed two or three times, at
the default launch size and at caps of 1 to 3 iterations per launch.  What ptmi_query.cpp, ptmi_guides.cpp and ptmi_denoise.cpp
promise in prose (they touch nothing but their planes; the calls that rewrite scene records wait for their stream first; the
filter reads the image ptmi_read_image would return) is what the model assumes.  One device: bit for bit.  Several: sample
counts, histograms and counters exactly, colour sums up to their association.  Hits and guide planes: bit for bit on any device
count (both run on devices[0] alone).  Filtered images: every word equal to denoise_cases.denoise of the image and the guide
planes the context returns, which are themselves held against the model, on any device count; through device pointers, of the
guide planes read back and the model's accumulators at the call (one device) or planes of the caller's.  The scripts, their
coverage and the model are checked without a GPU in test_api_fuzz_model.py."""
import os

import numpy as np
import pytest

from opencl_pathtracer_amd import Backend, backend, structs as S
import api_fuzz_cases as F
import guide_cases as G

pytestmark = pytest.mark.gpu


class DeviceIO:
    """ptmi_query_rays_device / ptmi_render_guides_device / ptmi_denoise_device on torch tensors on device 0.  No call is waited
    for: the result is collected (after ptmi_synchronize) when the executor asks, one operation later; the tensors live until then."""

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

        def collect():
            be.synchronize()
            for t, a in zip(sent, image or ()):
                assert np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32)), "denoise wrote an image plane of the caller's"
            return out.cpu().numpy(), {name: t.cpu().numpy() for name, t in guides.items()}

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
