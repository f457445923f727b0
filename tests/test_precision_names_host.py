"""The precision names the two models take, checked without a GPU: "f16x3_safe" (ABI value 3) is accepted by the
constructors and by set_precision, an unknown name is refused as before."""
import pytest

from acousticswarms_speech_amd.config import SEP_SMALL, SMALL
from acousticswarms_speech_amd.sep import SepModel
from acousticswarms_speech_amd.spot import SpotModel
from acousticswarms_speech_amd.weights import make_sep_state_dict, make_spot_state_dict


def test_spot_model_takes_f16x3_safe():
    sd = make_spot_state_dict(SMALL, 3)
    m = SpotModel(SMALL, sd, precision="f16x3_safe")
    assert m.precision == "f16x3_safe" and SpotModel.PRECISIONS["f16x3_safe"] == 3
    m.set_precision("f16x3")
    m.set_precision("f16x3_safe")
    assert m.precision == "f16x3_safe"
    with pytest.raises(RuntimeError):
        SpotModel(SMALL, sd, precision="f16x3_sfe")
    with pytest.raises(RuntimeError):
        m.set_precision("f16x3_sfe")
    assert m.precision == "f16x3_safe"


def test_sep_model_takes_f16x3_safe():
    sd = make_sep_state_dict(SEP_SMALL, 3)
    m = SepModel(SEP_SMALL, sd, precision="f16x3_safe")
    assert m.precision == "f16x3_safe" and SepModel.PRECISIONS["f16x3_safe"] == 3
    m.set_precision("f32")
    m.set_precision("f16x3_safe")
    with pytest.raises(RuntimeError):
        SepModel(SEP_SMALL, sd, precision="f16x3_sfe")
    with pytest.raises(RuntimeError):
        m.set_precision("f16x3_sfe")


def test_the_other_names_keep_their_values():
    for cls in (SpotModel, SepModel):
        assert {k: cls.PRECISIONS[k] for k in ("f32", "f16x3", "f16")} == {"f32": 0, "f16x3": 1, "f16": 2}


def test_library_exports_the_scaled_mask_path():
    """the C ABI: the new entry point exists beside the old one and the version is unchanged (additive change)"""
    from acousticswarms_speech_amd import native
    L = native.lib()
    assert L.asw_mask_path_f16x3_scaled is not None and L.asw_mask_path_f16x3 is not None
    assert L.asw_abi_version() == 3
