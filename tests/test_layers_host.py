"""Thickness series (MultisliceCalculator(layers=...)): the argument checks that run before any device work."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def traj():
    from pyslice_amd.synthetic import synthetic_trajectory
    return synthetic_trajectory(64, 6, 2, density=0.05, seed=4)


def _calc(**kw):
    from pyslice_amd.calculators import MultisliceCalculator
    return MultisliceCalculator(progress=False, **kw)


@pytest.mark.parametrize("layers", [[-1], [6], [0, 7], [1.5], ["2"], [True], [np.float64(2.0)], [None]])
def test_layers_validation_errors_from_setup(traj, layers):
    calc = _calc(layers=layers)
    with pytest.raises(ValueError, match="layer"):
        calc.setup(traj, aperture=30.0, voltage_eV=100e3)
    assert calc._engine is None


def test_layers_are_sorted_deduplicated_and_end_with_the_exit_wave():
    calc = _calc(layers=[3, 1, 1, np.int32(0), 5])
    assert calc._check_layers(6, 1) == [0, 1, 3, 5]
    assert calc._check_layers(8, 1) == [0, 1, 3, 5, 7]
    assert _calc(layers=[]).__dict__["_layers_arg"] == []
    assert _calc(layers=[])._check_layers(6, 1) == [5]
    assert _calc()._check_layers(6, 1) == [5]


def test_layers_refused_with_the_frame_cache_and_streaming():
    with pytest.raises(ValueError, match="cache"):
        _calc(layers=[0], cache=True)
    with pytest.raises(ValueError, match="stream_tile"):
        _calc(layers=[0], stream_tile=4)


def test_layers_refused_over_several_ranks(traj, monkeypatch):
    from pyslice_amd import distributed
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))
    calc = _calc(layers=[1])
    with pytest.raises(NotImplementedError, match="ranks"):
        calc.setup(traj, aperture=30.0, voltage_eV=100e3)
    assert calc._engine is None


def test_layer_buffer_and_entry_points_in_the_header_and_binding():
    from pyslice_amd import _native
    hdr = open(os.path.join(REPO, "include", "mslice.h")).read()
    assert re.search(r"MSL_BUF_LAYERS\s*=\s*11\b", hdr)
    assert _native.BUF_LAYERS == 11
    for name in ("msl_set_layers", "msl_download_layers_c128", "msl_tacaw_layer"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _native.EXPORTS
    assert re.search(r"#define\s+MSL_ABI_VERSION\s+3\b", hdr)
