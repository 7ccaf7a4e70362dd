"""The optional-member interface of the model types (drake_ddp_amd/csrc/model_traits.hpp), pinned: the value of each of the thirteen
traits for every built-in model of csrc/models.hpp and for the wrapper types LongHorizon<M>, ExactCost<M>, Limited<M>, as
static_asserts in one translation unit that includes csrc/launch_large.hpp.  Compile-only (-fsyntax-only): needs hipcc, no GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = ["Pendulum", "Acrobot", "CartPoleT<false>", "CartPoleT<true>", "Synth36", "PlanarQuad", "Quad3D", "Arm27", "Arm27C"]
# trait -> the built-in models on which it is on (models.hpp as it stands); off on every other one
ON = {
    "NewtonMeasured": ["Pendulum"],
    "HasStepPool": ["CartPoleT<true>"],
    "UsesScanBackward": [],
    "UsesExactBackward": [],
    "UsesLimits": [],
    "IsChainModel": ["PlanarQuad"],
    "IsLegModel": ["Quad3D"],
    "IsTrigModel": ["Arm27", "Arm27C"],
    "IsWholeStepModel": ["Arm27", "Arm27C"],
    "CanFail": ["PlanarQuad", "Quad3D"],
    "HasSparsity": ["Synth36"],
    "HasPivSplit": ["Synth36", "PlanarQuad", "Quad3D"],
}
EARLY_LEADER_BLOCKS = {"PlanarQuad": 1}          # the int trait; 0 on every other model

EXTRA = """
// the wrappers switch on their own member and keep the model's
static_assert(UsesScanBackward<LongHorizon<Acrobot>>::value && !UsesExactBackward<LongHorizon<Acrobot>>::value && !UsesLimits<LongHorizon<Acrobot>>::value);
static_assert(UsesExactBackward<ExactCost<Acrobot>>::value && !UsesScanBackward<ExactCost<Acrobot>>::value && !UsesLimits<ExactCost<Acrobot>>::value);
static_assert(UsesLimits<Limited<Pendulum>>::value && !UsesLimits<Pendulum>::value);
static_assert(!UsesScanBackward<Limited<Pendulum>>::value && !UsesExactBackward<Limited<Pendulum>>::value);
static_assert(NewtonMeasured<Limited<Pendulum>>::value);
static_assert(HasStepPool<Limited<CartPoleT<true>>>::value && HasStepPool<LongHorizon<CartPoleT<true>>>::value && !HasStepPool<Limited<CartPoleT<false>>>::value);
static_assert(UsesLimits<Limited<Arm27>>::value && IsTrigModel<Limited<Arm27>>::value && IsWholeStepModel<Limited<Arm27>>::value);
static_assert(!CanFail<Limited<Arm27C>>::value && !HasPivSplit<Limited<Arm27C>>::value && EarlyLeaderBlocks<Limited<Arm27C>>::value == 0);
static_assert(Limited<Pendulum>::n == 2 && Limited<Arm27>::m == 7 && LongHorizon<Acrobot>::n_params == 10 && ExactCost<Acrobot>::n == 4);
// the shapes of the detection: a bool member declared false is off, an int member gives its value, presence alone is on
struct Probe {
  static constexpr int n = 8, m = 13, n_params = 0;
  static constexpr bool kChainCooperative = false;
  static constexpr int kEarlyLeaderBlocks = 3;
  static constexpr int kMaxAffected = 0;
};
static_assert(!IsChainModel<Probe>::value && EarlyLeaderBlocks<Probe>::value == 3 && HasSparsity<Probe>::value);
static_assert(!IsLegModel<Probe>::value && !IsWholeStepModel<Probe>::value && !HasPivSplit<Probe>::value);
// the derived constants
static_assert(!kLxFromRollout<PlanarQuad> && kLxFromRollout<Synth36> && kLxFromRollout<Quad3D> && kLxFromRollout<Arm27>);
static_assert(kEarlyLin<Synth36> && kEarlyLin<Arm27> && !kEarlyLin<Probe>);
static_assert(kSpecRollout<Arm27> && kSpecRollout<Arm27C> && kSpecRollout<Limited<Arm27>>);
static_assert(!kSpecRollout<Synth36> && !kSpecRollout<PlanarQuad> && !kSpecRollout<Quad3D>);
static_assert(mi_host::kPivSplit<Synth36> && !mi_host::kPivSplit<Arm27>);
"""


def unit():
    lines = ['#include "launch_large.hpp"', "using namespace mi;"]
    for trait, on in ON.items():
        assert set(on) <= set(MODELS)
        for mdl in MODELS:
            lines.append("static_assert(%s%s<%s>::value, \"%s<%s>\");" % ("" if mdl in on else "!", trait, mdl, trait, mdl))
    for mdl in MODELS:
        lines.append("static_assert(EarlyLeaderBlocks<%s>::value == %d, \"EarlyLeaderBlocks<%s>\");" % (mdl, EARLY_LEADER_BLOCKS.get(mdl, 0), mdl))
    return "\n".join(lines) + EXTRA


def check(text, tmp_path):
    from drake_ddp_amd import build
    src = tmp_path / "model_traits_pins.hip"
    src.write_text(text)
    return subprocess.run([build.HIPCC] + build.FLAGS + ["-fsyntax-only", "-I", build.CSRC, str(src)],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_trait_values_of_every_builtin_model_and_wrapper(tmp_path):
    r = check(unit(), tmp_path)
    assert r.returncode == 0, r.stdout[-4000:]
