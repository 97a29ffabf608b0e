"""CPU: the host half of the self-guided band for tickets (dyn_aligner_set_auto_guide, Aligner.set_auto_guide,
dynamont-resquiggle --guide-auto / --guide-rounds). The entry point is declared and resolves within ABI 10; the switch is
range-checked with the texts the header promises, and 0 turns it off; the command's parser has train's names and defaults,
refuses the two pairings the library refuses, and takes --guide-rounds alone. (What a ticket under the switch computes needs
a device: tests/test_gpu_auto_guide_stream.py.)"""
import os
import re

import pytest

from conftest import ROOT
from dynamont_amd import Aligner
from dynamont_amd import _native as N
from dynamont_amd.segmentation import segment as seg_cli
from dynamont_amd.segmentation import train as train_cli

pytestmark = pytest.mark.usefixtures("native_lib")


def test_header_declares_the_entry_point_within_abi_10(native_lib):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    declared = set(re.findall(r"\b(dyn_[a-z0-9_]+)\s*\(", hdr))
    assert "dyn_aligner_set_auto_guide" in declared and "dyn_aligner_set_auto_guide" in N.SIGNATURES
    assert re.search(r"int dyn_aligner_set_auto_guide\(dyn_aligner\* a, uint32_t half_width, uint32_t max_rounds\);", hdr)
    assert getattr(native_lib, "dyn_aligner_set_auto_guide") is not None
    assert "DYN_ABI_VERSION 10" in hdr


def test_range_refusals_and_off(models):
    al = Aligner(models["syn5"], "dna_r9", device="host")
    try:
        assert al._auto_guide == (0, 8)
        for bad in (2047, 5000):
            with pytest.raises(ValueError, match=r"dyn_aligner_set_auto_guide: half_width %d is outside \[1, 2046\]" % bad):
                al.set_auto_guide(bad, 8)
        for bad in (0, 65):
            with pytest.raises(ValueError, match=r"dyn_aligner_set_auto_guide: max_rounds %d is outside \[1, 64\]" % bad):
                al.set_auto_guide(16, bad)
        assert al._auto_guide == (0, 8)                       # a refused call changes nothing
        for hw, rounds in ((1, 1), (2046, 64), (16, 8)):
            al.set_auto_guide(hw, rounds)
            assert al._auto_guide == (hw, rounds)
        al.set_auto_guide(0)                                  # off; max_rounds is not looked at
        assert al._auto_guide[0] == 0
        al.set_auto_guide(0, 0)
        assert N.lib().dyn_aligner_set_auto_guide(None, 16, 8) == N.DYN_ERR_INVALID_ARGUMENT
    finally:
        al.close()


BASE = ["-r", "raw", "-b", "calls.bam", "-o", "out", "--mode", "basic", "-p", "rna004"]


def test_parser_defaults_match_the_train_command():
    args = seg_cli.parse(BASE)
    assert (args.guide_auto, args.guide_rounds) == (0, 8)
    tr = train_cli.parse(["-r", "raw", "-b", "calls.bam", "-o", "out", "-p", "rna004"])
    assert (tr.guide_auto, tr.guide_rounds) == (args.guide_auto, args.guide_rounds)
    args = seg_cli.parse(BASE + ["--guide-auto", "16", "--guide-rounds", "4", "--event-stats", "--segment-scores", "8",
                                 "--kmer-summary", "k.tsv", "--band-report", "b.tsv", "--host-preprocess"])
    assert (args.guide_auto, args.guide_rounds) == (16, 4)


@pytest.mark.parametrize("other, name", [(["--rescale-iters", "2"], "--rescale-iters"), (["--border-confidence", "8"], "--border-confidence")])
def test_parser_refuses_what_the_library_refuses(other, name, capsys):
    with pytest.raises(SystemExit) as e:
        seg_cli.parse(BASE + ["--guide-auto", "16"] + other)
    assert e.value.code == 2
    assert "--guide-auto and %s are mutually exclusive" % name in capsys.readouterr().err
    assert seg_cli.parse(BASE + other).guide_auto == 0        # without the flag the other switch is accepted


def test_guide_rounds_alone_is_accepted_and_ignored():
    args = seg_cli.parse(BASE + ["--guide-rounds", "3"])
    assert (args.guide_auto, args.guide_rounds) == (0, 3)
    args = seg_cli.parse(BASE + ["--guide-rounds", "3", "--rescale-iters", "1"])
    assert args.guide_auto == 0 and args.rescale_iters == 1
