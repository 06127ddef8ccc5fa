#!/usr/bin/env python3
"""Golden files for the file-format functions of effi_mvs_plus_amd/gipuma.py, produced by RUNNING the reference's own misc/gipuma.py
-- write_gipuma_dmb, mvsnet_to_gipuma_dmb, mvsnet_to_gipuma_cam, fake_gipuma_normal, probability_filter -- and recording the BYTES
it wrote, next to the inputs it was given:
  * a 1-channel and a 3-channel .dmb (the 3-channel one planar: the reference transposes to [c][h][w] before writing);
  * a .P file from a DTU-style _cam.txt (the float64 product K [R|t], each entry as str(float64));
  * the fake-normal .dmb of the 1-channel depth (1 / 1.732050808 where the depth is positive);
  * a _prob_filtered.pfm.
The reference module imports ``datasets.data_io`` (its PFM reader / writer); only that FILE of the reference's ``datasets`` package is
loaded, under a stub package; the modules it imports for functions never called here (torchvision, cv2: both absent) are stubbed.
Run from the repo root:  python tests/golden/make_golden_gipuma.py
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

CAM_TXT = """extrinsic
0.970263 0.00747983 0.241939 -191.02
-0.0147429 0.999493 0.0282234 3.28832
-0.241605 -0.030951 0.969881 22.5401
0.0 0.0 0.0 1.0

intrinsic
2892.33 0 823.205
0 2883.18 619.071
0 0 1

425 2.5
"""


def load_reference():
    sys.dont_write_bytecode = True
    pkg = types.ModuleType("datasets")
    pkg.__path__ = []
    sys.modules["datasets"] = pkg
    # data_io.py imports torchvision.transforms and cv2 at module level for functions this script never calls; both are absent here
    for name in ("torchvision", "torchvision.transforms", "cv2"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    for name, path in (("datasets.data_io", "datasets/data_io.py"), ("ref_misc_gipuma", "misc/gipuma.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules["ref_misc_gipuma"], sys.modules["datasets.data_io"]


def raw(path):
    with open(path, "rb") as f:
        return np.frombuffer(f.read(), np.uint8).copy()


def main():
    G, IO = load_reference()
    rng = np.random.default_rng(18)
    h, w = 11, 14
    depth = (rng.random((h, w), dtype=np.float32) * 500 + 400).astype(np.float32)
    depth[2:5, 3:9] = 0.0
    depth[7, 1] = -3.0
    conf = rng.random((h, w), dtype=np.float32)
    img3 = rng.random((h, w, 3), dtype=np.float32)
    out = dict(depth=depth, conf=conf, img3=img3, cam_txt=np.frombuffer(CAM_TXT.encode(), np.uint8).copy(), prob_threshold=np.float64(0.35))
    with tempfile.TemporaryDirectory() as tmp:
        p = lambda *a: os.path.join(tmp, *a)
        G.write_gipuma_dmb(p("one.dmb"), depth)
        G.write_gipuma_dmb(p("three.dmb"), img3)
        out["dmb1"], out["dmb3"] = raw(p("one.dmb")), raw(p("three.dmb"))
        out["dmb1_read"] = np.ascontiguousarray(G.read_gipuma_dmb(p("one.dmb")))
        with open(p("00000003_cam.txt"), "w") as f:
            f.write(CAM_TXT)
        G.mvsnet_to_gipuma_cam(p("00000003_cam.txt"), p("00000003.jpg.P"))
        out["cam_P"] = raw(p("00000003.jpg.P"))
        G.fake_gipuma_normal(p("one.dmb"), p("normals.dmb"))
        out["normals"] = raw(p("normals.dmb"))
        # probability_filter on a one-view dense folder, then the .pfm -> .dmb conversion of its result
        for sub in ("images", "depth_est", "confidence"):
            os.mkdir(p(sub))
        open(p("images", "00000003.jpg"), "wb").close()
        IO.save_pfm(p("depth_est", "00000003.pfm"), depth)
        IO.save_pfm(p("confidence", "00000003.pfm"), conf)
        out["depth_pfm"], out["conf_pfm"] = raw(p("depth_est", "00000003.pfm")), raw(p("confidence", "00000003.pfm"))
        G.probability_filter(p(), 0.35)
        out["prob_filtered_pfm"] = raw(p("depth_est", "00000003_prob_filtered.pfm"))
        G.mvsnet_to_gipuma_dmb(p("depth_est", "00000003_prob_filtered.pfm"), p("disp.dmb"))
        out["disp_dmb"] = raw(p("disp.dmb"))
    import inspect
    for fn in ("read_gipuma_dmb", "write_gipuma_dmb", "mvsnet_to_gipuma_dmb", "mvsnet_to_gipuma_cam", "fake_gipuma_normal", "mvsnet_to_gipuma",
               "probability_filter", "read_camera_parameters", "gipuma_filter"):
        out[f"sig_{fn}"] = np.asarray([str(inspect.signature(getattr(G, fn)))])
    path = os.path.join(HERE, "g18_gipuma_io.npz")
    np.savez_compressed(path, **out)
    print(f"g18_gipuma_io.npz: {os.path.getsize(path) / 1024:.1f} KiB; .P file:\n{out['cam_P'].tobytes().decode()}")


if __name__ == "__main__":
    main()
