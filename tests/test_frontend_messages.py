"""What the front end's argument checks refuse, in which words, and what they return for what they accept - frozen from the commit
before drake_ddp_amd/ilqr.py was split into argcheck.py, results.py and ilqr.py.  CPU only, no built library.

REFUSED: (check function, its arguments as source, the exact message).  METHODS: the same for the refusals of the classes that
are reachable on an object made with object.__new__, which has no handle.  ACCEPTED: arguments whose results - values, dtype, shape,
contiguity - are in tests/frontend_accepted.json.  Both the messages and that file are what the earlier commit answered:

    git worktree add /tmp/parent <that commit>
    PYTHONPATH=/tmp/parent python tests/test_frontend_messages.py --record tests/frontend_accepted.json

writes the file and prints every row of REFUSED and METHODS whose message differs from what that checkout raises (none)."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.dirname(HERE))
sys.path.insert(0, HERE)

from frontend_fake import encode  # noqa: E402

# B = 3 problems; n = 2 states, m = 3 controls (m_dev = 4 where padding is asked for), n_params = 2, N = 10
REFUSED = [
    # ---- check_model_params(params, B, n_params)
    ("check_model_params", "[1.0], 3, 0", "SetModelParameters: this model has no parameters"),
    ("check_model_params", "'ab', 3, 2", "SetModelParameters: not an array of numbers (could not convert string to float: 'ab')"),
    ("check_model_params", "np.zeros((2, 2)), 3, 2", "SetModelParameters: parameters must be (3, 2) or (2,); got (2, 2)"),
    ("check_model_params", "[1.0, nan], 3, 2", "SetModelParameters: NaN or infinity"),
    ("check_model_params", "[[1.0, inf]] * 3, 3, 2", "SetModelParameters: NaN or infinity"),
    # ---- check_target_trajectory(x_ref, clock, B, n)
    ("check_target_trajectory", "None, -1, 3, 2", "SetTargetTrajectory: clock must be an integer in [0, 2^30); got -1"),
    ("check_target_trajectory", "None, 1.5, 3, 2", "SetTargetTrajectory: clock must be an integer in [0, 2^30); got 1.5"),
    ("check_target_trajectory", "None, 'a', 3, 2", "SetTargetTrajectory: clock must be an integer in [0, 2^30); got 'a'"),
    ("check_target_trajectory", "None, 2 ** 30, 3, 2", "SetTargetTrajectory: clock must be an integer in [0, 2^30); got 1073741824"),
    ("check_target_trajectory", "None, inf, 3, 2", "SetTargetTrajectory: clock must be an integer in [0, 2^30); got inf"),
    ("check_target_trajectory", "'ab', 0, 3, 2", "SetTargetTrajectory: not an array of numbers (could not convert string to float: 'ab')"),
    ("check_target_trajectory", "np.zeros((4, 3)), 0, 3, 2", "SetTargetTrajectory: the reference must be (T, 2) or (3, T, 2); got (4, 3)"),
    ("check_target_trajectory", "np.zeros((2, 4, 2)), 0, 3, 2", "SetTargetTrajectory: the reference must be (T, 2) or (3, T, 2); got (2, 4, 2)"),
    ("check_target_trajectory", "np.zeros((0, 2)), 0, 3, 2", "SetTargetTrajectory: the reference needs at least one row (T >= 1)"),
    ("check_target_trajectory", "np.full((4, 2), inf), 0, 3, 2", "SetTargetTrajectory: NaN or infinity"),
    # ---- check_rollout_args(x0, params, B, n, n_params)
    ("check_rollout_args", "'ab', None, 3, 2, 2", "RolloutPolicy: x0 is not an array of numbers (could not convert string to float: 'ab')"),
    ("check_rollout_args", "np.zeros((5, 3)), None, 3, 2, 2", "RolloutPolicy: x0 must be (3, S, 2) or (S, 2) with S >= 1; got (5, 3)"),
    ("check_rollout_args", "np.zeros((0, 2)), None, 3, 2, 2", "RolloutPolicy: x0 must be (3, S, 2) or (S, 2) with S >= 1; got (0, 2)"),
    ("check_rollout_args", "np.zeros((5, 2)), [1.0], 3, 2, 0", "RolloutPolicy: this model has no parameters"),
    ("check_rollout_args", "np.zeros((5, 2)), 'ab', 3, 2, 2", "RolloutPolicy: params is not an array of numbers (could not convert string to float: 'ab')"),
    ("check_rollout_args", "np.zeros((5, 2)), np.zeros((4, 2)), 3, 2, 2", "RolloutPolicy: params must be (3, 5, 2) or (5, 2); got (4, 2)"),
    ("check_rollout_args", "np.zeros((5, 2)), np.full((5, 2), nan), 3, 2, 2", "RolloutPolicy: NaN or infinity in params"),
    # ---- check_noise_args(state_noise, control_noise, seed, first_sample, common_noise, B, n, m, m_dev=None, S=None)
    ("check_noise_args", "None, None, 'a', 0, False, 3, 2, 3", "RolloutPolicy: seed must be an integer in [0, 2^53); got 'a'"),
    ("check_noise_args", "None, None, True, 0, False, 3, 2, 3", "RolloutPolicy: seed must be an integer in [0, 2^53); got True"),
    ("check_noise_args", "None, None, 1.5, 0, False, 3, 2, 3", "RolloutPolicy: seed must be an integer in [0, 2^53); got 1.5"),
    ("check_noise_args", "None, None, nan, 0, False, 3, 2, 3", "RolloutPolicy: seed must be an integer in [0, 2^53); got nan"),
    ("check_noise_args", "None, None, -1, 0, False, 3, 2, 3", "RolloutPolicy: seed must be an integer in [0, 2^53); got -1"),
    ("check_noise_args", "None, None, 2.0 ** 53, 0, False, 3, 2, 3", "RolloutPolicy: seed must be an integer in [0, 2^53); got 9007199254740992"),
    ("check_noise_args", "None, None, 0, 2 ** 32, False, 3, 2, 3", "RolloutPolicy: first_sample must be an integer in [0, 2^32); got 4294967296"),
    ("check_noise_args", "None, None, 0, None, False, 3, 2, 3", "RolloutPolicy: first_sample must be an integer in [0, 2^32); got None"),
    ("check_noise_args", "None, None, 0, 2 ** 32 - 4, False, 3, 2, 3, None, 5", "RolloutPolicy: first_sample + S must not exceed 2^32; got 4294967292 + 5"),
    ("check_noise_args", "'ab', None, 0, 0, False, 3, 2, 3", "RolloutPolicy: state_noise is not an array of numbers (could not convert string to float: 'ab')"),
    ("check_noise_args", "np.zeros(3), None, 0, 0, False, 3, 2, 3", "RolloutPolicy: state_noise must be a scalar, (2,) or (3, 2); got (3,)"),
    ("check_noise_args", "None, np.zeros((3, 4)), 0, 0, False, 3, 2, 3, 4", "RolloutPolicy: control_noise must be a scalar, (3,) or (3, 3); got (3, 4)"),
    ("check_noise_args", "inf, None, 0, 0, False, 3, 2, 3", "RolloutPolicy: NaN or infinity in state_noise"),
    ("check_noise_args", "None, [0.0, nan, 0.0], 0, 0, False, 3, 2, 3", "RolloutPolicy: NaN or infinity in control_noise"),
    ("check_noise_args", "None, -1.0, 0, 0, False, 3, 2, 3", "RolloutPolicy: negative entry in control_noise (standard deviations)"),
    # ---- check_plant_args(x, params, state_noise, control_noise, seed, common_noise, feedback, clock, B, n, m, n_params, m_dev=None)
    ("check_plant_args", "'ab', None, None, None, 0, False, True, 0, 3, 2, 3, 2", "SetPlant: x is not an array of numbers (could not convert string to float: 'ab')"),
    ("check_plant_args", "np.zeros(3), None, None, None, 0, False, True, 0, 3, 2, 3, 2", "SetPlant: x must be (3, 2) or (2,); got (3,)"),
    ("check_plant_args", "[0.0, nan], None, None, None, 0, False, True, 0, 3, 2, 3, 2", "SetPlant: NaN or infinity in x"),
    ("check_plant_args", "[0.0, 0.0], [1.0], None, None, 0, False, True, 0, 3, 2, 3, 0", "SetPlant: this model has no parameters"),
    ("check_plant_args", "[0.0, 0.0], [[1.0]], None, None, 0, False, True, 0, 3, 2, 3, 2", "SetPlant: params must be (3, 2) or (2,); got (1, 1)"),
    ("check_plant_args", "[0.0, 0.0], [1.0, inf], None, None, 0, False, True, 0, 3, 2, 3, 2", "SetPlant: NaN or infinity in params"),
    ("check_plant_args", "[0.0, 0.0], ['a', 'b'], None, None, 0, False, True, 0, 3, 2, 3, 2", "SetPlant: params is not an array of numbers (could not convert string to float: 'a')"),
    ("check_plant_args", "[0.0, 0.0], None, None, None, 0, False, True, -1, 3, 2, 3, 2", "SetPlant: clock must be an integer in [0, 2^32); got -1"),
    ("check_plant_args", "[0.0, 0.0], None, None, None, 0, False, True, 0.5, 3, 2, 3, 2", "SetPlant: clock must be an integer in [0, 2^32); got 0.5"),
    ("check_plant_args", "[0.0, 0.0], None, None, None, 0, False, True, 2.0 ** 32, 3, 2, 3, 2", "SetPlant: clock must be an integer in [0, 2^32); got 4294967296"),
    ("check_plant_args", "[0.0, 0.0], None, None, None, 'a', False, True, 0, 3, 2, 3, 2", "SetPlant: seed must be an integer in [0, 2^53); got 'a'"),
    ("check_plant_args", "[0.0, 0.0], None, None, None, -3, False, True, 0, 3, 2, 3, 2", "SetPlant: seed must be an integer in [0, 2^53); got -3"),
    ("check_plant_args", "[0.0, 0.0], None, None, None, 2 ** 53, False, True, 0, 3, 2, 3, 2", "SetPlant: seed must be an integer in [0, 2^53); got 9007199254740992"),
    ("check_plant_args", "[0.0, 0.0], None, [1.0], None, 0, False, True, 0, 3, 2, 3, 2", "SetPlant: state_noise must be a scalar, (2,) or (3, 2); got (1,)"),
    ("check_plant_args", "[0.0, 0.0], None, None, -0.5, 0, False, True, 0, 3, 2, 3, 2, 4", "SetPlant: negative entry in control_noise (standard deviations)"),
    ("check_plant_args", "[0.0, 0.0], None, None, 'ab', 0, False, True, 0, 3, 2, 3, 2", "SetPlant: control_noise is not an array of numbers (could not convert string to float: 'ab')"),
    ("check_plant_args", "[0.0, 0.0], None, nan, None, 0, False, True, 0, 3, 2, 3, 2", "SetPlant: NaN or infinity in state_noise"),
    ("check_plant_args", "[0.0, 0.0], None, None, None, 0, 2, True, 0, 3, 2, 3, 2", "SetPlant: common_noise must be True or False; got 2"),
    ("check_plant_args", "[0.0, 0.0], None, None, None, 0, False, 1.0, 0, 3, 2, 3, 2", "SetPlant: feedback must be True or False; got 1.0"),
    ("check_plant_args", "[0.0, 0.0], None, None, None, 0, False, None, 0, 3, 2, 3, 2", "SetPlant: feedback must be True or False; got None"),
    # ---- check_mc_args(S, x0_mean, x0_spread, B, n, n_params, *, x0_dist, params_mean, params_spread, params_dist, goal, samples, first_sample)
    ("check_mc_args", "0, [0.0, 0.0], [1.0, 1.0], 3, 2, 2", "RolloutPolicyStats: S must be an integer >= 1; got 0"),
    ("check_mc_args", "4.0, [0.0, 0.0], [1.0, 1.0], 3, 2, 2", "RolloutPolicyStats: S must be an integer >= 1; got 4.0"),
    ("check_mc_args", "True, [0.0, 0.0], [1.0, 1.0], 3, 2, 2", "RolloutPolicyStats: S must be an integer >= 1; got True"),
    ("check_mc_args", "4, [0.0, 0.0], [1.0, 1.0], 3, 2, 2, first_sample=2.0", "RolloutPolicyStats: first_sample must be an integer in [0, 2^32); got 2.0"),
    ("check_mc_args", "4, [0.0, 0.0], [1.0, 1.0], 3, 2, 2, first_sample=-1", "RolloutPolicyStats: first_sample must be an integer in [0, 2^32); got -1"),
    ("check_mc_args", "4, [0.0, 0.0], [1.0, 1.0], 3, 2, 2, first_sample=2 ** 32 - 2", "RolloutPolicyStats: first_sample + S must not exceed 2^32; got 4294967294 + 4"),
    ("check_mc_args", "4, [0.0, 0.0], [1.0, 1.0], 3, 2, 2, x0_dist='cauchy'", "RolloutPolicyStats: x0_dist must be 'normal' or 'uniform'; got 'cauchy'"),
    ("check_mc_args", "4, [0.0, 0.0], [1.0, 1.0], 3, 2, 2, params_dist=None", "RolloutPolicyStats: params_dist must be 'normal' or 'uniform'; got None"),
    ("check_mc_args", "4, 'ab', [1.0, 1.0], 3, 2, 2", "RolloutPolicyStats: x0_mean is not an array of numbers (could not convert string to float: 'ab')"),
    ("check_mc_args", "4, [0.0, 0.0, 0.0], [1.0, 1.0], 3, 2, 2", "RolloutPolicyStats: x0_mean must be (2,) or (3, 2); got (3,)"),
    ("check_mc_args", "4, [0.0, inf], [1.0, 1.0], 3, 2, 2", "RolloutPolicyStats: NaN or infinity in x0_mean"),
    ("check_mc_args", "4, [0.0, 0.0], [1.0, nan], 3, 2, 2", "RolloutPolicyStats: NaN or infinity in x0_spread"),
    ("check_mc_args", "4, [0.0, 0.0], [1.0, -1.0], 3, 2, 2", "RolloutPolicyStats: negative entry in x0_spread"),
    ("check_mc_args", "4, [0.0, 0.0], [1.0, 1.0], 3, 2, 2, goal=[nan, 1.0]", "RolloutPolicyStats: NaN in goal"),
    ("check_mc_args", "4, [0.0, 0.0], [1.0, 1.0], 3, 2, 2, goal=[inf, -1.0]", "RolloutPolicyStats: negative entry in goal"),
    ("check_mc_args", "4, [0.0, 0.0], [1.0, 1.0], 3, 2, 2, goal=1.0", "RolloutPolicyStats: goal must be (2,) or (3, 2); got ()"),
    ("check_mc_args", "4, [0.0, 0.0], [1.0, 1.0], 3, 2, 2, params_spread=[1.0, 1.0]", "RolloutPolicyStats: params_spread needs params_mean"),
    ("check_mc_args", "4, [0.0, 0.0], [1.0, 1.0], 3, 2, 0, params_mean=[]", "RolloutPolicyStats: this model has no parameters"),
    ("check_mc_args", "4, [0.0, 0.0], [1.0, 1.0], 3, 2, 2, params_mean=[1.0]", "RolloutPolicyStats: params_mean must be (2,) or (3, 2); got (1,)"),
    ("check_mc_args", "4, [0.0, 0.0], [1.0, 1.0], 3, 2, 2, params_mean=[1.0, 1.0], params_spread=[-1.0, 0.0]", "RolloutPolicyStats: negative entry in params_spread"),
    # ---- check_mc_observe(envelope, controls, safe_box, B, n)
    ("check_mc_observe", "1, False, None, 3, 2", "RolloutPolicyStats: envelope must be True or False; got 1"),
    ("check_mc_observe", "True, None, None, 3, 2", "RolloutPolicyStats: controls must be True or False; got None"),
    ("check_mc_observe", "False, False, [1.0, 2.0, 3.0], 3, 2", "RolloutPolicyStats: safe_box must be a pair (lo, hi)"),
    ("check_mc_observe", "False, False, np.zeros((2, 2)), 3, 2", "RolloutPolicyStats: safe_box must be a pair (lo, hi)"),
    ("check_mc_observe", "False, False, ('ab', None), 3, 2", "RolloutPolicyStats: safe_box lo is not an array of numbers (could not convert string to float: 'ab')"),
    ("check_mc_observe", "False, False, (None, [1.0]), 3, 2", "RolloutPolicyStats: safe_box hi must be (2,) or (3, 2); got (1,)"),
    ("check_mc_observe", "False, False, ([nan, 0.0], None), 3, 2", "RolloutPolicyStats: NaN in safe_box lo"),
    ("check_mc_observe", "False, False, ([0.0, 1.0], [1.0, 0.5]), 3, 2", "RolloutPolicyStats: safe_box has lo > hi"),
    # ---- check_seed_args(K, B, m, sigma_u=None, seed=0, round=0, hold=1, m_dev=None, what="PerturbInitialGuess")
    ("check_seed_args", "0, 3, 3", "PerturbInitialGuess: K must be an integer in [1, 2^31); got 0"),
    ("check_seed_args", "1.5, 3, 3, what='SelectBest'", "SelectBest: K must be an integer in [1, 2^31); got 1.5"),
    ("check_seed_args", "True, 3, 3", "PerturbInitialGuess: K must be an integer in [1, 2^31); got True"),
    ("check_seed_args", "2, 3, 3, what='GatherBest'", "GatherBest: K must divide the batch: 3 problems are no whole number of groups of 2"),
    ("check_seed_args", "3, 3, 3, None, -1", "PerturbInitialGuess: seed must be an integer in [0, 2^53); got -1"),
    ("check_seed_args", "3, 3, 3, None, 2.0 ** 53", "PerturbInitialGuess: seed must be an integer in [0, 2^53); got 9007199254740992.0"),
    ("check_seed_args", "3, 3, 3, None, 0, 2 ** 32", "PerturbInitialGuess: round must be an integer in [0, 2^32); got 4294967296"),
    ("check_seed_args", "3, 3, 3, None, 0, 0, 0", "PerturbInitialGuess: hold must be an integer in [1, 2^31); got 0"),
    ("check_seed_args", "3, 3, 3, None, 0, 0, inf", "PerturbInitialGuess: hold must be an integer in [1, 2^31); got inf"),
    ("check_seed_args", "3, 3, 3, 'ab'", "PerturbInitialGuess: sigma_u is not an array of numbers (could not convert string to float: 'ab')"),
    ("check_seed_args", "3, 3, 3, [1.0, 2.0], what='ReseedFromBest'", "ReseedFromBest: sigma_u must be a scalar, (3,) or (3, 3); got (2,)"),
    ("check_seed_args", "3, 3, 3, nan", "PerturbInitialGuess: NaN or infinity in sigma_u"),
    ("check_seed_args", "3, 3, 3, [1.0, -1.0, 0.0]", "PerturbInitialGuess: negative entry in sigma_u (standard deviations)"),
    # ---- check_mppi_args(S, iterations, B, m, N, sigma_u, temperature, seed=0, first_sample=0, hold=1, shift=0, m_dev=None, what="MPPIRun")
    ("check_mppi_args", "0, 2, 3, 3, 10, 0.5, 1.0", "MPPIRun: S must be an integer in [1, 2^31 - 64]; got 0"),
    ("check_mppi_args", "2 ** 31 - 63, 2, 3, 3, 10, 0.5, 1.0", "MPPIRun: S must be an integer in [1, 2^31 - 64]; got 2147483585"),
    ("check_mppi_args", "8, 0.5, 3, 3, 10, 0.5, 1.0", "MPPIRun: iterations must be an integer in [1, 2^31); got 0.5"),
    ("check_mppi_args", "8, 2, 3, 3, 10, None, 1.0", "MPPIRun: sigma_u is required"),
    ("check_mppi_args", "8, 2, 3, 3, 10, [0.5], 1.0", "MPPIRun: sigma_u must be a scalar, (3,) or (3, 3); got (1,)"),
    ("check_mppi_args", "8, 2, 3, 3, 10, -0.5, 1.0", "MPPIRun: negative entry in sigma_u (standard deviations)"),
    ("check_mppi_args", "8, 2, 3, 3, 10, 0.5, 1.0, -1", "MPPIRun: seed must be an integer in [0, 2^53); got -1"),
    ("check_mppi_args", "8, 2, 3, 3, 10, 0.5, 1.0, 0, 0, 0", "MPPIRun: hold must be an integer in [1, 2^31); got 0"),
    ("check_mppi_args", "8, 2, 3, 3, 10, 0.5, 1.0, 0, 2 ** 32", "MPPIRun: first_sample must be an integer in [0, 2^32); got 4294967296"),
    ("check_mppi_args", "8, 2, 3, 3, 10, 0.5, 1.0, 0, 2 ** 32 - 15", "MPPIRun: first_sample + iterations S must not exceed 2^32 (iteration i draws samples first_sample + i S ..)"),
    ("check_mppi_args", "8, 2, 3, 3, 10, 0.5, 1.0, 0, 0, 1, 9", "MPPIRun: shift must be an integer in [0, 8]; got 9"),
    ("check_mppi_args", "8, 2, 3, 3, 10, 0.5, 1.0, 0, 0, 1, -1, None, 'Sampler'", "Sampler: shift must be an integer in [0, 8]; got -1"),
    ("check_mppi_args", "8, 2, 3, 3, 10, 0.5, -1.0", "MPPIRun: temperature must be a number >= 0 (0: the best sample alone); got -1.0"),
    ("check_mppi_args", "8, 2, 3, 3, 10, 0.5, nan", "MPPIRun: temperature must be a number >= 0 (0: the best sample alone); got nan"),
    ("check_mppi_args", "8, 2, 3, 3, 10, 0.5, '1'", "MPPIRun: temperature must be a number >= 0 (0: the best sample alone); got '1'"),
    ("check_mppi_args", "8, 2, 3, 3, 10, 0.5, True", "MPPIRun: temperature must be a number >= 0 (0: the best sample alone); got True"),
    # ---- two bad arguments at once: which one is reported is behaviour
    ("check_target_trajectory", "'ab', -1, 3, 2", "SetTargetTrajectory: clock must be an integer in [0, 2^30); got -1"),
    ("check_rollout_args", "np.zeros((5, 3)), 'ab', 3, 2, 0", "RolloutPolicy: x0 must be (3, S, 2) or (S, 2) with S >= 1; got (5, 3)"),
    ("check_noise_args", "-1.0, None, -1, -1, False, 3, 2, 3", "RolloutPolicy: seed must be an integer in [0, 2^53); got -1"),
    ("check_noise_args", "-1.0, None, 0, -1, False, 3, 2, 3", "RolloutPolicy: first_sample must be an integer in [0, 2^32); got -1"),
    ("check_noise_args", "-1.0, nan, 0, 0, False, 3, 2, 3", "RolloutPolicy: negative entry in state_noise (standard deviations)"),
    ("check_plant_args", "[0.0, nan], [1.0], -1.0, None, -1, 2, 2, -1, 3, 2, 3, 0", "SetPlant: NaN or infinity in x"),
    ("check_plant_args", "[0.0, 0.0], [1.0, nan], -1.0, None, -1, 2, 2, -1, 3, 2, 3, 2", "SetPlant: NaN or infinity in params"),
    ("check_plant_args", "[0.0, 0.0], None, -1.0, None, -1, 2, 2, -1, 3, 2, 3, 2", "SetPlant: seed must be an integer in [0, 2^53); got -1"),
    ("check_plant_args", "[0.0, 0.0], None, -1.0, None, 0, 2, 2, -1, 3, 2, 3, 2", "SetPlant: clock must be an integer in [0, 2^32); got -1"),
    ("check_plant_args", "[0.0, 0.0], None, -1.0, None, 0, 2, 2, 0, 3, 2, 3, 2", "SetPlant: negative entry in state_noise (standard deviations)"),
    ("check_plant_args", "[0.0, 0.0], None, None, None, 0, 2, 2, 0, 3, 2, 3, 2", "SetPlant: common_noise must be True or False; got 2"),
    ("check_mc_args", "0, 'ab', [1.0, 1.0], 3, 2, 2, first_sample=-1, x0_dist='x'", "RolloutPolicyStats: S must be an integer >= 1; got 0"),
    ("check_mc_args", "4, 'ab', [1.0, 1.0], 3, 2, 2, first_sample=-1, x0_dist='x'", "RolloutPolicyStats: first_sample must be an integer in [0, 2^32); got -1"),
    ("check_mc_args", "4, 'ab', [1.0, 1.0], 3, 2, 2, x0_dist='x'", "RolloutPolicyStats: x0_dist must be 'normal' or 'uniform'; got 'x'"),
    ("check_mc_args", "4, [0.0, 0.0], [-1.0, 1.0], 3, 2, 0, goal=[nan, 0.0], params_spread=[1.0]", "RolloutPolicyStats: negative entry in x0_spread"),
    ("check_mc_args", "4, [0.0, 0.0], [1.0, 1.0], 3, 2, 0, goal=[nan, 0.0], params_spread=[1.0]", "RolloutPolicyStats: NaN in goal"),
    ("check_mc_args", "4, [0.0, 0.0], [1.0, 1.0], 3, 2, 0, params_spread=[1.0]", "RolloutPolicyStats: params_spread needs params_mean"),
    ("check_mc_observe", "1, 1, 3, 3, 2", "RolloutPolicyStats: envelope must be True or False; got 1"),
    ("check_mc_observe", "False, False, ([nan, 0.0], [1.0]), 3, 2", "RolloutPolicyStats: NaN in safe_box lo"),
    ("check_seed_args", "2, 3, 3, -1.0, -1, -1, 0", "PerturbInitialGuess: K must divide the batch: 3 problems are no whole number of groups of 2"),
    ("check_seed_args", "3, 3, 3, -1.0, -1, -1, 0", "PerturbInitialGuess: seed must be an integer in [0, 2^53); got -1"),
    ("check_seed_args", "3, 3, 3, -1.0, 0, -1, 0", "PerturbInitialGuess: round must be an integer in [0, 2^32); got -1"),
    ("check_seed_args", "3, 3, 3, -1.0, 0, 0, 0", "PerturbInitialGuess: hold must be an integer in [1, 2^31); got 0"),
    ("check_mppi_args", "0, 0, 3, 3, 10, None, -1.0", "MPPIRun: S must be an integer in [1, 2^31 - 64]; got 0"),
    ("check_mppi_args", "8, 0, 3, 3, 10, None, -1.0", "MPPIRun: iterations must be an integer in [1, 2^31); got 0"),
    ("check_mppi_args", "8, 2, 3, 3, 10, -0.5, -1.0, -1, -1, 0, -1", "MPPIRun: seed must be an integer in [0, 2^53); got -1"),
    ("check_mppi_args", "8, 2, 3, 3, 10, -0.5, -1.0, 0, -1, 0, -1", "MPPIRun: hold must be an integer in [1, 2^31); got 0"),
    ("check_mppi_args", "8, 2, 3, 3, 10, -0.5, -1.0, 0, -1, 1, -1", "MPPIRun: negative entry in sigma_u (standard deviations)"),
    ("check_mppi_args", "8, 2, 3, 3, 10, 0.5, -1.0, 0, -1, 1, -1", "MPPIRun: first_sample must be an integer in [0, 2^32); got -1"),
    ("check_mppi_args", "8, 2, 3, 3, 10, 0.5, -1.0, 0, 0, 1, -1", "MPPIRun: shift must be an integer in [0, 8]; got -1"),
]

# (class, method, arguments, message) on an object without a handle: B = 3 (the drop-in class: 1), n = 2, m = 3, m_dev = 4, N = 10,
# two model parameters, control_limits="enforce"
METHODS = [
    ("BatchedIterativeLQR", "SolveMultiStart", "3, 0, 0.5", "SolveMultiStart: rounds must be an integer >= 1; got 0"),
    ("BatchedIterativeLQR", "SolveMultiStart", "3, 2.0, 0.5", "SolveMultiStart: rounds must be an integer >= 1; got 2.0"),
    ("BatchedIterativeLQR", "SolveMultiStart", "3, True, 0.5", "SolveMultiStart: rounds must be an integer >= 1; got True"),
    ("BatchedIterativeLQR", "SolveMultiStart", "3, 2, 0.5, shrink=-1.0", "SolveMultiStart: shrink must be a finite number >= 0; got -1.0"),
    ("BatchedIterativeLQR", "SolveMultiStart", "3, 2, 0.5, shrink=inf", "SolveMultiStart: shrink must be a finite number >= 0; got inf"),
    ("BatchedIterativeLQR", "SolveMultiStart", "3, 2, 0.5, shrink='1'", "SolveMultiStart: shrink must be a finite number >= 0; got '1'"),
    ("BatchedIterativeLQR", "SolveMultiStart", "3, 2, None", "SolveMultiStart: sigma_u is required"),
    ("BatchedIterativeLQR", "SolveMultiStart", "2, 0, None", "SolveMultiStart: rounds must be an integer >= 1; got 0"),
    ("BatchedIterativeLQR", "SolveMultiStart", "2, 2, None", "SolveMultiStart: K must divide the batch: 3 problems are no whole number of groups of 2"),
    ("BatchedIterativeLQR", "MPCRunMultiStart", "3, 0, 1, 0.5", "MPCRunMultiStart: num_resolves must be an integer in [1, 2147483648); got 0"),
    ("BatchedIterativeLQR", "MPCRunMultiStart", "3, 2.0, 1, 0.5", "MPCRunMultiStart: num_resolves must be an integer in [1, 2147483648); got 2.0"),
    ("BatchedIterativeLQR", "MPCRunMultiStart", "3, 2, 9, 0.5", "MPCRunMultiStart: replan_steps must be an integer in [1, 9); got 9"),
    ("BatchedIterativeLQR", "MPCRunMultiStart", "3, 2, True, 0.5", "MPCRunMultiStart: replan_steps must be an integer in [1, 9); got True"),
    ("BatchedIterativeLQR", "MPCRunMultiStart", "3, 0, 0, None", "MPCRunMultiStart: sigma_u is required"),
    ("BatchedIterativeLQR", "MPCRunMultiStart", "3, 0, 0, 0.5", "MPCRunMultiStart: num_resolves must be an integer in [1, 2147483648); got 0"),
    ("BatchedIterativeLQR", "MPCRunMultiStart", "3, 2, 1, 0.5, round=2 ** 32 - 1", "MPCRunMultiStart: round + num_resolves must not exceed 2^32 (re-solve r draws at round + r)"),
    ("BatchedIterativeLQR", "PerturbInitialGuess", "3, None", "PerturbInitialGuess: sigma_u is required"),
    ("BatchedIterativeLQR", "ReseedFromBest", "3, None", "ReseedFromBest: sigma_u is required"),
    ("BatchedIterativeLQR", "ReseedFromBest", "3, None, -1", "ReseedFromBest: seed must be an integer in [0, 2^53); got -1"),
    ("BatchedIterativeLQR", "SelectBest", "2", "SelectBest: K must divide the batch: 3 problems are no whole number of groups of 2"),
    ("BatchedIterativeLQR", "GatherBest", "0", "GatherBest: K must be an integer in [1, 2^31); got 0"),
    ("BatchedIterativeLQR", "SetControlLimits", "None, [1.0, 1.0, 1.0]", "SetControlLimits: give both bounds, or (None, None) to clear them"),
    ("BatchedIterativeLQR", "SetControlLimits", "[0.0, 0.0], [1.0, 1.0, 1.0]", "SetControlLimits: u_min (2,) and u_max (3,) differ in shape"),
    ("BatchedIterativeLQR", "SetControlLimits", "0.0, 1.0", "SetControlLimits: bounds must be scalars (m = 1), (3,) or (3, 3); got ()"),
    ("BatchedIterativeLQR", "SetControlLimits", "np.zeros((2, 3)), np.ones((2, 3))", "SetControlLimits: bounds must be scalars (m = 1), (3,) or (3, 3); got (2, 3)"),
    ("BatchedIterativeLQR", "SetControlLimits", "[0.0, nan, 0.0], [1.0, 1.0, 1.0]", "SetControlLimits: u_min > u_max or NaN"),
    ("BatchedIterativeLQR", "SetControlLimits", "[0.0, 2.0, 0.0], [1.0, 1.0, 1.0]", "SetControlLimits: u_min > u_max or NaN"),
    ("BatchedIterativeLQR", "SetPlant", "[0.0, 0.0], clock=-1, seed=-1", "SetPlant: seed must be an integer in [0, 2^53); got -1"),
    ("BatchedIterativeLQR", "SetPlant", "[0.0, 0.0], clock=2 ** 32", "SetPlant: clock must be an integer in [0, 2^32); got 4294967296"),
    ("BatchedIterativeLQR", "RolloutPolicy", "np.zeros((5, 2)), first_sample=-1", "RolloutPolicy: first_sample must be an integer in [0, 2^32); got -1"),
    ("BatchedIterativeLQR", "RolloutPolicyStats", "4.0, [0.0, 0.0], [1.0, 1.0]", "RolloutPolicyStats: S must be an integer >= 1; got 4.0"),
    ("BatchedIterativeLQR", "MPPIRun", "8, 2, 0.5, -1.0", "MPPIRun: temperature must be a number >= 0 (0: the best sample alone); got -1.0"),
    ("BatchedIterativeLQR", "SetModelParameters", "[1.0]", "SetModelParameters: parameters must be (3, 2) or (2,); got (1,)"),
    ("BatchedIterativeLQR", "SetTargetTrajectory", "np.zeros((4, 2)), -1", "SetTargetTrajectory: clock must be an integer in [0, 2^30); got -1"),
    ("IterativeLinearQuadraticRegulator", "RolloutPolicy", "np.zeros((1, 5, 2))", "RolloutPolicy: x0 must be (S, 2); got (1, 5, 2)"),
    ("IterativeLinearQuadraticRegulator", "RolloutPolicy", "np.zeros(2)", "RolloutPolicy: x0 must be (S, 2); got (2,)"),
    ("IterativeLinearQuadraticRegulator", "SetTargetTrajectory", "np.zeros((1, 4, 2))", "SetTargetTrajectory: the reference must be (T, 2); got (1, 4, 2)"),
    ("IterativeLinearQuadraticRegulator", "SetTargetTrajectory", "np.zeros((4, 2)), 0.5", "SetTargetTrajectory: clock must be an integer in [0, 2^30); got 0.5"),
    ("IterativeLinearQuadraticRegulator", "SetPlant", "np.zeros((1, 2))", "SetPlant: x must be (2,); got (1, 2)"),
    ("IterativeLinearQuadraticRegulator", "SetPlant", "np.zeros(2), np.zeros((1, 2))", "SetPlant: params must be (2,); got (1, 2)"),
    ("IterativeLinearQuadraticRegulator", "SetPlant", "np.zeros(2), clock=0.5", "SetPlant: clock must be an integer in [0, 2^32); got 0.5"),
]

# accepted: (check function, arguments); what each returns is in frontend_accepted.json under "<function>(<arguments>)"
ACCEPTED = [
    ("check_model_params", "None, 3, 2"),
    ("check_model_params", "None, 3, 0"),
    ("check_model_params", "[1.0, 2.0], 3, 2"),
    ("check_model_params", "np.arange(6.0).reshape(2, 3).T, 3, 2"),
    ("check_model_params", "np.arange(6).reshape(3, 2), 3, 2"),
    ("check_target_trajectory", "None, 5, 3, 2"),
    ("check_target_trajectory", "None, np.int32(7), 3, 2"),
    ("check_target_trajectory", "None, 3.0, 3, 2"),
    ("check_target_trajectory", "np.arange(8.0).reshape(4, 2), 2 ** 30 - 1, 3, 2"),
    ("check_target_trajectory", "np.arange(24.0).reshape(2, 4, 3).T, True, 3, 2"),
    ("check_rollout_args", "np.arange(10.0).reshape(5, 2), None, 3, 2, 2"),
    ("check_rollout_args", "np.arange(10.0).reshape(5, 2), None, 3, 2, 0"),
    ("check_rollout_args", "np.full((3, 1, 2), nan), np.arange(2.0).reshape(1, 2), 3, 2, 2"),
    ("check_rollout_args", "np.arange(30).reshape(3, 5, 2), np.arange(30.0).reshape(2, 5, 3).T, 3, 2, 2"),
    ("check_noise_args", "None, None, 0, 0, False, 3, 2, 3"),
    ("check_noise_args", "None, None, np.int64(2 ** 53 - 1), 2.0 ** 32 - 1, 1, 3, 2, 3, None, 1"),
    ("check_noise_args", "None, None, np.float32(4.0), np.uint8(3), 'yes', 3, 2, 3, 4, np.int16(2)"),
    ("check_noise_args", "0.5, None, 1, 2, True, 3, 2, 3"),
    ("check_noise_args", "None, 0.25, 1, 2, False, 3, 2, 3, 4"),
    ("check_noise_args", "[0.5, 0.0], [0.25, 0.5, 1.0], 1, 2, False, 3, 2, 3, 4, 9"),
    ("check_noise_args", "np.arange(6.0).reshape(3, 2), np.arange(9).reshape(3, 3), 3.0, 4.0, False, 3, 2, 3, 4"),
    ("check_plant_args", "[0.5, 0.25], None, None, None, 0, False, True, 0, 3, 2, 3, 2"),
    ("check_plant_args", "np.arange(6.0).reshape(2, 3).T, [1.0, 2.0], 0.5, None, 7, 1, 0, 9.0, 3, 2, 3, 2, 4"),
    ("check_plant_args", "np.arange(6).reshape(3, 2), np.arange(6.0).reshape(3, 2), [0.5, 0.0], np.arange(9.0).reshape(3, 3), np.int32(7), "
                         "np.bool_(True), np.int64(1), np.uint32(2 ** 32 - 1), 3, 2, 3, 2, 4"),
    ("check_plant_args", "[0.5, 0.25], None, None, None, 0, False, True, 0, 3, 2, 3, 0"),
    ("check_mc_args", "4, [0.0, 1.0], [0.5, 0.25], 3, 2, 2"),
    ("check_mc_args", "np.int32(4), np.arange(6.0).reshape(3, 2), [0.5, 0.0], 3, 2, 2, x0_dist='uniform', goal=[inf, 0.5], samples=1, "
                      "first_sample=np.int64(2 ** 32 - 4)"),
    ("check_mc_args", "4, [0.0, 1.0], [0.5, 0.25], 3, 2, 2, params_mean=[1.0, 2.0], params_dist='normal'"),
    ("check_mc_args", "4, [0.0, 1.0], [0.5, 0.25], 3, 2, 2, params_mean=np.arange(6.0).reshape(3, 2), params_spread=[0.5, 0.0], goal=np.ones((3, 2))"),
    ("check_mc_args", "1, [0.0, 1.0], [0.5, 0.25], 3, 2, 0"),
    ("check_mc_observe", "False, False, None, 3, 2"),
    ("check_mc_observe", "True, np.bool_(True), None, 3, 2"),
    ("check_mc_observe", "False, True, (None, None), 3, 2"),
    ("check_mc_observe", "True, False, ([-inf, 0.0], None), 3, 2"),
    ("check_mc_observe", "False, False, [np.arange(6.0).reshape(3, 2), [inf, 9.0]], 3, 2"),
    ("check_mc_observe", "False, False, ([1.0, 1.0], [1.0, 1.0]), 3, 2"),
    ("check_seed_args", "3, 3, 3"),
    ("check_seed_args", "np.int64(1), 3, 3, None, 2.0 ** 53 - 1, np.uint32(2 ** 32 - 1), 3.0, what='SelectBest'"),
    ("check_seed_args", "3.0, 3, 3, 0.5, 1, 2, 3"),
    ("check_seed_args", "3, 3, 3, 0.5, 1, 2, 3, 4"),
    ("check_seed_args", "1, 3, 3, [0.5, 0.25, 0.0], m_dev=4"),
    ("check_seed_args", "1, 3, 3, np.arange(9).reshape(3, 3), m_dev=4"),
    ("check_mppi_args", "8, 2, 3, 3, 10, 0.5, 1.0"),
    ("check_mppi_args", "2 ** 31 - 64, 1.0, 3, 3, 10, [0.5, 0.25, 0.0], 0, 2.0 ** 53 - 1, 2 ** 31, np.int16(4), 8.0, 4"),
    ("check_mppi_args", "np.int32(8), np.int64(2), 3, 3, 10, np.arange(9.0).reshape(3, 3), np.float32(0.5), 1, 2 ** 32 - 16, 2, 0, 4, 'X'"),
    ("check_mppi_args", "8, 2, 3, 3, 10, 0.5, inf"),
    ("check_mppi_args", "8, 2, 3, 3, 10, 0.5, 3"),
]

RETURNS = {}
if __name__ != "__main__":
    with open(os.path.join(HERE, "frontend_accepted.json")) as _f:
        RETURNS = json.load(_f)

NAMES = {"np": np, "nan": np.nan, "inf": np.inf}


def call(function, arguments):
    from drake_ddp_amd import ilqr
    return eval(f"f({arguments})", dict(NAMES, f=getattr(ilqr, function)))   # noqa: S307


def call_method(cls, method, arguments):
    """The method on an object that has no handle and no library: whatever it raises, it raises before it touches either."""
    from drake_ddp_amd import ilqr

    class _System:
        params = np.array([0.25, 0.5])

    s = object.__new__(getattr(ilqr, cls))
    s.B, s.n, s.m, s._md, s.N, s.system = (1 if cls == "IterativeLinearQuadraticRegulator" else 3), 2, 3, 4, 10, _System()
    s.control_limits = "enforce"
    return eval(f"f({arguments})", dict(NAMES, f=getattr(s, method)))   # noqa: S307


def message_of(f, *a):
    try:
        f(*a)
    except ValueError as e:
        return str(e)
    return None


def test_every_check_function_and_enough_rows():
    assert {r[0] for r in REFUSED} == {r[0] for r in ACCEPTED} == {
        "check_model_params", "check_target_trajectory", "check_rollout_args", "check_noise_args", "check_plant_args", "check_mc_args",
        "check_mc_observe", "check_seed_args", "check_mppi_args"}
    assert len(REFUSED) >= 55 and len(set(REFUSED)) == len(REFUSED)


@pytest.mark.parametrize("function,arguments,message", REFUSED)
def test_refused_with_the_same_words(function, arguments, message):
    assert message_of(call, function, arguments) == message


@pytest.mark.parametrize("cls,method,arguments,message", METHODS)
def test_methods_refuse_with_the_same_words_before_they_touch_a_handle(cls, method, arguments, message):
    assert message_of(call_method, cls, method, arguments) == message


@pytest.mark.parametrize("function,arguments", ACCEPTED)
def test_accepted_returns_the_same(function, arguments):
    """encode() writes an array as dtype, shape, C-contiguity and the hex of every element: equal records are np.array_equal arrays
    (NaN equal to NaN) of the same dtype, shape and layout; ints, floats and None compare as themselves."""
    assert json.loads(json.dumps(encode(call(function, arguments)))) == RETURNS[f"{function}({arguments})"]


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_frontend_messages.py --record FILE")
    for row in REFUSED:
        if message_of(call, *row[:2]) != row[2]:
            print(row[:2], repr(message_of(call, *row[:2])))
    for row in METHODS:
        if message_of(call_method, *row[:3]) != row[3]:
            print(row[:3], repr(message_of(call_method, *row[:3])))
    with open(sys.argv[2], "w") as f:
        json.dump({f"{fn}({a})": encode(call(fn, a)) for fn, a in ACCEPTED}, f, indent=0, separators=(",", ":"))
        f.write("\n")
