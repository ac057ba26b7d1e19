"""The temporal entries write the bits of the build that tests/golden/temporal_bits.json was recorded on
(tools/record_temporal_bits.py; the commit is in the file): k_denoise_temporal, k_denoise_temporal_motion,
k_denoise_temporal_alpha and k_gradient_alpha_camera over the chains of tests/temporal_bits_cases.py, every frame's linear
film, RGBA8 film or alpha plane (NaN entries as their bits) by SHA-256."""
import json
import os

import pytest

import temporal_bits_cases as B

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "temporal_bits.json")


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_the_fixture_holds_every_case(recorded):
    assert sorted(recorded) == sorted(B.key(n, W, H) for n in B.CASES for W, H in B.SIZES)


@pytest.mark.parametrize("size", B.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", B.CASES)
def test_temporal_entries_write_the_recorded_bits(pt, gpu_ctx, recorded, name, size):
    got = B.digests(B.run(pt, gpu_ctx, name, *size))
    want = recorded[B.key(name, *size)]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, size, "frame", k)
