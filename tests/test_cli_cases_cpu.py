"""The host side of the command line against the record of the tree as it was before the run settings got their one table, the
cameras their one source and main() its per-command functions (tests/golden/cli_cases.json, tools/record_cli_cases.py): what the
sub-commands parse to, what make_run_state records and _resolve_run_settings resolves, how a capture is read, the text of every
argparse error that ends a command line before the GPU is asked for, the cameras the resolvers return, and what main() hands to
train().  No flag, default, message or checkpoint key may move.  No GPU: nothing is loaded onto one and nothing is launched."""
import io
import json
import os

import pytest

from tests.helpers import GOLDEN
from tools import record_cli_cases as rec


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLDEN, "cli_cases.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    """The record of the tree, made in a directory of its own (every path in a message is relative to it) and passed through the
    recorder's own writer, as the committed file was."""
    here = os.getcwd()
    os.chdir(tmp_path_factory.mktemp("cli_cases"))
    try:
        text = io.StringIO()
        rec.dump(rec.record(), text)
    finally:
        os.chdir(here)
    return text.getvalue()


def test_the_record_has_every_group_and_command(pinned):
    assert tuple(sorted(pinned)) == tuple(sorted(rec.GROUPS))
    assert set(pinned["parses"]) == {f"{c} {which} run_defaults={d}" for c in rec.PARSES for which in ("minimal", "full") for d in (True, False)}
    assert set(pinned["main_errors"]) == {" ".join(argv) for argv in rec.MAIN_ERRORS} and all(pinned["main_errors"].values())
    assert pinned["parses"]["train minimal run_defaults=True"]["scale_factor"] == rec.NOT_GIVEN
    assert pinned["parses"]["train full run_defaults=True"]["scale_factor"] == 0.5


@pytest.mark.parametrize("group", rec.GROUPS)
def test_the_tree_computes_what_the_record_holds(pinned, recorded, group):
    got = json.loads(recorded)[group]
    assert set(got) == set(pinned[group])
    for name in pinned[group]:
        assert got[name] == pinned[group][name], name


def test_the_recorder_reproduces_the_file_byte_for_byte(recorded):
    with open(os.path.join(GOLDEN, "cli_cases.json")) as fh:
        assert recorded == fh.read()
