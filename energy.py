#!/usr/bin/env python3
"""examples/energy.jl on MI355X: the energy drift of the pendulum's GP rollout (600 000 recorded
steps, and the 1000-step pair with 20 and 10 samples) against explicit Euler, written to an .npz.
See gpr.jl_amd/gprx/energy.py.

    python energy.py [--steps 600000 --short-steps 1000 --seed 1 --out energy.npz]
"""
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent
sys.path[:0] = [str(REPO), str(REPO / "gpr.jl_amd")]

from gprx.energy import main  # noqa: E402

if __name__ == "__main__":
    main()
