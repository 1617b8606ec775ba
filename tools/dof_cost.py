"""Cost of a thin-lens frame: bench.py's flagship workload (the 1 M-triangle height field, 1920 x 1080, 4 spp, diffuse variant) rendered
with frames in flight, once with the pinhole camera and once with aperture_radius > 0 -- which routes the frame through the general
kernel instantiations (csrc/host_frame.inl path_kernel_flags). Prints ms per frame for both, each measured `--repeat` times alternating.

focus_distance is the distance from the camera to the point it looks at (the middle of the height field)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from realtimepathtracingresearchframework_amd import abi, backend, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--aperture", type=float, default=0.05)
    ap.add_argument("--frames-in-flight", type=int, default=3)
    args = ap.parse_args()
    W, H, spp = 1920, 1080, 4
    s = scenes.grid_1m()
    focus = float(np.linalg.norm(np.asarray(s.camera["center"], np.float64) - np.asarray(s.camera["eye"], np.float64)))
    r = backend.RenderHip(frames_in_flight=args.frames_in_flight)
    r.initialize(W, H)
    r.set_scene(s)
    cam = s.camera_params()

    def run(aperture, n):
        r.params.aperture_radius = aperture
        r.params.focus_distance = focus
        queue = []
        for _ in range(n):
            queue.append(r.render_async(backend.RenderConfiguration(cam, active_variant=abi.VARIANT_SIMPLE, reset_accumulation=False), spp=spp))
            if len(queue) >= args.frames_in_flight:
                r.wait(queue.pop(0))
        while queue:
            r.wait(queue.pop(0))

    out = {"pinhole_ms": [], "lens_ms": []}
    for _ in range(args.repeat):
        for key, aperture in (("pinhole_ms", 0.0), ("lens_ms", args.aperture)):
            run(aperture, args.warmup)
            t0 = time.perf_counter()
            run(aperture, args.steps)
            out[key].append(round((time.perf_counter() - t0) * 1e3 / args.steps, 4))
    out.update(aperture_radius=args.aperture, focus_distance=round(focus, 4), width=W, height=H, spp=spp, frames_in_flight=args.frames_in_flight,
               steps=args.steps, warmup=args.warmup)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
