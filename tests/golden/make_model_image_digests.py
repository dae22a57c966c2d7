"""Generate tests/golden/model_image_digests.json: the SHA-256 of gpu.model_image (the 28 KB
psgpu::DevModel the kernels read, built on the host by psgpu_model_build.h) for every synth
config and for the fuzz parity seeds (tests/test_gpu_fuzz.py fuzz_case).

Every byte of the image matters: set_model compares images to decide "same model", and the
graph key and the JIT cache hang off it.  tests/test_host.py checks the built library against
these digests; psgpu_model_image needs no device.

Usage: python tests/golden/make_model_image_digests.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from parsip_amd import gpu, synth  # noqa: E402
from test_gpu_fuzz import fuzz_case  # noqa: E402

FUZZ_SEEDS = range(40)


def models():
    for name in sorted(synth.CONFIGS):
        yield name, synth.make_config(name)[0]
    for seed in FUZZ_SEEDS:
        yield f"fuzz{seed}", fuzz_case(seed)[0]


def digest(model) -> str:
    return hashlib.sha256(gpu.model_image(model)).hexdigest()


if __name__ == "__main__":
    out = {"generator": "gpu.model_image of synth.make_config(name) and test_gpu_fuzz.fuzz_case(seed)",
           "models": {name: digest(m) for name, m in models()}}
    print(len(out["models"]), "models")
    with open(os.path.join(HERE, "model_image_digests.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
