"""Loads a component script (``<comp>/<comp>.py``) as a module, for the tests of its flag surface and its functions."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_component(comp):
    spec = importlib.util.spec_from_file_location(comp + "_cli", os.path.join(ROOT, comp, comp + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod
