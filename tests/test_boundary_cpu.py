"""The plugin boundary on CPU: PredictionType answers compare equal to the reference's
own enum (the reference's train_step / gen.py dispatch on them), and the C-ABI-free
parts of the drop-in contract (prediction types of every model class)."""
import enum
import json
import os

from ensemble_svs_with_interactions_amd import base
from ensemble_svs_with_interactions_amd.base import PredictionType

REF_ENUM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                        "prediction_type.json")


def _ref_enum():
    # the reference's enum is a plain enum.Enum (no overridden methods): rebuilt from its
    # recorded class name, module and members (tests/golden/prediction_type.json)
    with open(REF_ENUM) as f:
        rec = json.load(f)
    return enum.Enum(rec["class"], rec["members"], module=rec["module"])


def test_prediction_type_equals_reference_enum():
    Ref = _ref_enum()
    for name in ("DETERMINISTIC", "PROBABILISTIC", "MULTISTREAM_HYBRID", "DIFFUSION"):
        ours, ref = getattr(PredictionType, name), getattr(Ref, name)
        assert ours == ref and ref == ours
        assert not (ours != ref)
        assert ours in [ref] and ref in [ours]
        assert hash(ours) == hash(ref)
        assert {ref: 1}[ours] == 1
    assert PredictionType.DIFFUSION != Ref.MULTISTREAM_HYBRID
    assert Ref.DETERMINISTIC != PredictionType.PROBABILISTIC


def test_reference_dispatch_branch():
    """train_acoustic_multitrack.py:120 takes the multistream branch for our model."""
    Ref = _ref_enum()
    from ensemble_svs_with_interactions_amd import configs
    model = configs.instantiate(configs.multitrack_diffusion(num_speakers=4, tiny=True))
    assert model.prediction_type() == Ref.MULTISTREAM_HYBRID
    assert model.mgc_model.prediction_type() == Ref.DIFFUSION
    assert model.vuv_model.prediction_type() == Ref.DETERMINISTIC
    assert model.has_residual_lf0_prediction() and model.is_autoregressive()


def test_fallback_enum_is_used_without_nnsvs():
    # this container has no importable nnsvs: the fallback enum is the one exported
    assert PredictionType is base._PredictionType or PredictionType.__module__ == "nnsvs.base"
