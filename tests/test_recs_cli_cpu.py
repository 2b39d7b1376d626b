"""The command-line plumbing the model_recs family shares (anime_recommendations_amd/cli.py): the flag lists, the user
pick, the CSV-and-artifact a run leaves behind and the ``__main__`` tail.  No GPU."""
import argparse
import logging
import random

import pandas as pd
import pytest

from component_cli import load_component
from anime_recommendations_amd import artifacts, cli, components as C

FAMILY = ["model_recs", "diverse_recs", "calibrated_recs", "explain_recs", "group_recs"]


@pytest.fixture
def workdir(tmp_path, monkeypatch):
    """An empty working directory and artifact store; the root logger's handlers (``setup_logging`` replaces them) are
    put back afterwards."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("ANIREC_ARTIFACT_DIR", str(tmp_path / "store"))
    root = logging.getLogger()
    handlers, level = root.handlers[:], root.level
    yield tmp_path
    for h in root.handlers[:]:
        root.removeHandler(h)
        h.close()
    for h in handlers:
        root.addHandler(h)
    root.setLevel(level)


def test_the_family_shares_one_flag_set(workdir):
    assert len(cli.MODEL_RECS_STR_FLAGS) == 17 and len(cli.MODEL_RECS_BOOL_FLAGS) == 6
    for comp in FAMILY:
        mod = load_component(comp)
        assert mod.STR_FLAGS == cli.MODEL_RECS_STR_FLAGS and mod.BOOL_FLAGS == cli.MODEL_RECS_BOOL_FLAGS, comp
    mod = load_component("new_user_recs")
    assert mod.STR_FLAGS == cli.MODEL_RECS_STR_FLAGS + ["new_ratings", "fold_steps", "fold_lr"]
    assert mod.BOOL_FLAGS == cli.MODEL_RECS_BOOL_FLAGS + ["fold_neighbours"]
    assert cli.MODEL_RECS_STR_FLAGS[-1] == "flow_ID_type" and cli.MODEL_RECS_BOOL_FLAGS[-1] == "model_ID_conf"   # not grown in place


@pytest.mark.parametrize("comp", FAMILY)
def test_select_user(comp, workdir):
    mod = load_component(comp)
    df = pd.DataFrame({"user_id": [7, 7, 9, 11, 9], "anime_id": [1, 2, 1, 3, 4], "rating": [.1, .2, .3, .4, .5]})
    pd.DataFrame({"User_ID": [9]}).to_csv("9.csv", index=False)
    artifacts.log_artifact("user_id.csv", "9.csv", "csv")
    ns = argparse.Namespace(model_ID_flow=True, model_ID_conf=True, model_user_query="11", flow_ID="user_id.csv:latest",
                            flow_ID_type="csv")
    user = mod.select_user(ns, df)
    assert user == 9 and type(user) is int                      # the flow's user wins over the configured one
    ns.model_ID_flow = False
    user = mod.select_user(ns, df)
    assert user == 11 and type(user) is int
    ns.model_ID_conf = False
    random.seed(0)
    want = random.choice([7, 9, 11])
    random.seed(0)
    user = mod.select_user(ns, df)
    assert user == want and type(user) is int


def _frame():
    return pd.DataFrame({"Name": ["A", "B, the second", "C"], "Prediction": [0.75, 0.5, 0.25], "anime_id": [5, 3, 8]})


@pytest.mark.parametrize("save", [True, False])
def test_write_recs(save, workdir):
    frame, fn = _frame(), "User_ID_7_recs.csv"
    metadata = {"Queried user: ": 7, "Filename": fn, "pool": 100, "floor": None, "members": [7, 9]}
    ns = argparse.Namespace(model_recs_type="recs_csv", save_model_recs=save)
    assert cli.write_recs(ns, frame, fn, "recs.csv", "three rows", metadata) is frame
    assert (workdir / fn).exists() == save
    if save:
        pd.testing.assert_frame_equal(pd.read_csv(workdir / fn), frame, check_exact=True)
    stored = artifacts.use_artifact("recs.csv:latest", "recs_csv")
    assert stored.endswith(fn)
    pd.testing.assert_frame_equal(pd.read_csv(stored), frame, check_exact=True)
    assert artifacts.artifact_metadata("recs.csv:latest") == metadata


def test_run_logs_the_failure_and_raises_it(workdir, monkeypatch):
    logger = C.setup_logging("some_recs")
    parser = argparse.ArgumentParser()
    parser.add_argument("--n", type=int, required=True)
    monkeypatch.setattr("sys.argv", ["some_recs.py", "--n", "3"])
    seen = []

    def go(args):
        seen.append(args.n)
        raise KeyError("no such anime")

    with pytest.raises(KeyError, match="no such anime"):
        cli.run("some_recs", logger, go, parser)
    assert seen == [3]
    for h in logger.handlers:
        h.flush()
    log = (workdir / "some_recs.log").read_text()
    assert "ERROR - some_recs failed" in log and "KeyError: 'no such anime'" in log
    seen.clear()
    cli.run("some_recs", logger, lambda args: seen.append(args.n), parser)      # a clean run logs nothing
    assert seen == [3] and (workdir / "some_recs.log").read_text() == log
