"""BeamCTCDecoder's limits: beams up to 128 over up to 64 labels (the reference's Cyrillic
label set of 36 at its default beam of 100 is inside them).  No GPU."""
import os

import pytest

from oracle import ds2_oracle as orc

EXTRA = "0123456789абвгдежзийклмнопрстуфхцч"
ARPA = os.path.join(os.path.dirname(__file__), "golden", "tiny_lm.arpa")


def WIDE(n):
    return orc.LABELS + EXTRA[:n]


def test_wide_label_sets():
    assert len(WIDE(3)) == 33 and len(WIDE(6)) == 36 and len(WIDE(34)) == 64
    assert WIDE(34)[0] == '_' and ' ' in WIDE(34)


def test_reference_defaults_over_36_labels():
    from ds2amd.decoder import BeamCTCDecoder
    dec = BeamCTCDecoder(WIDE(6))
    assert dec.beam_width == 100
    assert len(dec.labels) == 36


def test_both_maxima_construct():
    from ds2amd.decoder import BeamCTCDecoder
    dec = BeamCTCDecoder(WIDE(34), beam_width=128)
    assert dec.beam_width == 128 and len(dec.labels) == 64


@pytest.mark.parametrize("labels", [orc.LABELS, WIDE(6), WIDE(34)])
def test_beam_129_raises(labels):
    from ds2amd.decoder import BeamCTCDecoder
    with pytest.raises(ValueError, match="128"):
        BeamCTCDecoder(labels, beam_width=129)


@pytest.mark.parametrize("beam", [1, 32, 100])
def test_65_labels_raise(beam):
    from ds2amd.decoder import BeamCTCDecoder
    with pytest.raises(ValueError, match="64"):
        BeamCTCDecoder(WIDE(34) + "ш", beam_width=beam)


def test_arpa_scorer_over_64_labels():
    from ds2amd.lm import ArpaScorer
    scorer = ArpaScorer(ARPA, WIDE(34), 0.8, 1.0, device="cpu")
    assert scorer.dict_next.shape[1] == 64
