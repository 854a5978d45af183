"""Optimizers — mirror of src/optimizer.{h,cc}: SGD + momentum (the optimizer of the target configs) and the two second-moment
optimizers built on it, Adagrad and RMSProp, each with a one-pass fused step (include/convnet_hip.h).  LBFGS and shared_prior are out of
scope."""
import collections
import ctypes
import math

import numpy as np

from .matrix import Matrix


_libm = None


def _expf(x):
    """The C library's expf — the function the reference's `exp(float)` resolves to (numpy's float32 exp is a different
    implementation and may differ in the last bit).  libm is located at first use; on a platform without one the float32 numpy
    value is used."""
    global _libm
    if _libm is None:
        import ctypes.util
        try:
            lm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
            lm.expf.restype, lm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
            _libm = lm
        except (OSError, AttributeError):
            _libm = False
    if _libm:
        return np.float32(_libm.expf(float(x)))
    return np.exp(np.float32(x), dtype=np.float32)


class Optimizer:
    @staticmethod
    def ChooseOptimizer(config):
        # src/optimizer.cc:8-29
        if config.optimizer_type == "STOCHASTIC_GRADIENT_DESCENT":
            return SGDOptimizer(config)
        if config.optimizer_type == "ADAGRAD_SGD":
            return AdagradSGDOptimizer(config)
        if config.optimizer_type == "RMSPROP_SGD":
            return RMSPropSGDOptimizer(config)
        raise SystemExit(f"Undefined optimizer {config.optimizer_type} (SGD, Adagrad and RMSProp are built; LBFGS is out of scope).")

    def __init__(self, c):
        self.epsilon_decay_type_ = c.epsilon_decay
        self.epsilon_ = c.epsilon
        self.minimum_epsilon_ = c.minimum_epsilon
        self.decay_factor_ = c.decay_factor
        self.epsilon_decay_timescale_ = c.epsilon_decay_timescale
        self.start_optimization_after_ = c.start_optimization_after
        self.l2_decay_ = c.l2_decay
        self.weight_norm_limit_ = c.weight_norm_limit
        self.weight_norm_constraint_ = c.weight_norm_constraint
        self.step_ = 0
        if c.shared_prior:
            raise SystemExit("shared_prior is out of scope")

    def ReduceLearningRate(self, factor):
        self.epsilon_ *= factor

    def ApplyConstraints(self, parameter):
        # src/optimizer.cc:75-81 (axis=1: per output unit)
        if self.weight_norm_constraint_ > 0:
            parameter.NormLimitByAxis(1, self.weight_norm_constraint_, True)
        elif self.weight_norm_limit_ > 0:
            parameter.NormLimitByAxis(1, self.weight_norm_limit_, False)

    def GetDecayedEpsilon(self):
        # src/optimizer.cc:83-104, evaluated in the reference's types: `float f`, expf, float arithmetic; only EXPONENTIAL_STEP
        # goes through double (C++11 pow(float, int) promotes both) and is rounded to float once.  Intentional deviation: for decay
        # type NONE with a timescale > 0 the reference's guard (it compares the TIMESCALE with the enum NONE, :85-86) enters the
        # branch and exits with "Unknown epsilon decay rule"; here that combination just means "no decay".
        f32 = np.float32
        eps = f32(self.epsilon_)
        ts = self.epsilon_decay_timescale_
        if ts > 0 and self.epsilon_decay_type_ != "NONE":
            f = f32(f32(self.step_) / f32(ts))
            t = self.epsilon_decay_type_
            if t == "EXPONENTIAL":
                eps = f32(f32(self.epsilon_) * _expf(-f))
            elif t == "INVERSE_T":
                eps = f32(f32(self.epsilon_) / f32(f32(1) + f))
            elif t == "LINEAR":
                eps = f32(f32(f32(self.epsilon_) * f32(f32(1) - f)) + f32(f32(self.minimum_epsilon_) * f)) if f < 1 else f32(self.minimum_epsilon_)
            elif t == "EXPONENTIAL_STEP":
                eps = f32(float(f32(self.epsilon_)) * math.pow(float(f32(self.decay_factor_)), self.step_ // ts))
            else:
                raise SystemExit("Unknown epsilon decay rule.")
        return float(max(eps, f32(self.minimum_epsilon_)))

    def NotifyStart(self, parameter):
        pass

    def AllocateMemory(self, rows, cols, storage=None, storage2=None):
        pass

    def NeedsSecondHistory(self):
        return False

    def IsAllocated(self):
        return False

    def LoadParameters(self, file, prefix):     # src/optimizer.cc:110-111: the base class stores nothing
        pass

    def SaveParameters(self, file, prefix):
        pass


# A plain fused step as DATA, per optimizer kind: the arguments of the kind's Matrix.*MomentumStep, and `multi`, the launch that runs a
# list of them (one launch per 16 tensors).  PlanFusedStep returns one; RunFusedSteps launches a step's collection, one multi launch per kind.
class SGDStep(collections.namedtuple("SGDStep", "gradient parameter history l2_decay gradient_clip epsilon momentum")):
    multi = staticmethod(lambda items: Matrix.SGDMomentumStepMulti(items))


class AdagradStep(collections.namedtuple("AdagradStep", "gradient parameter history adagrad_history delta step_scale l2_decay gradient_clip "
                                                        "epsilon momentum")):
    multi = staticmethod(lambda items: Matrix.AdagradMomentumStepMulti(items))


class RMSPropStep(collections.namedtuple("RMSPropStep", "gradient parameter history rms_history factor l2_decay gradient_clip epsilon momentum")):
    multi = staticmethod(lambda items: Matrix.RMSPropMomentumStepMulti(items))


def RunFusedSteps(items):
    """The planned steps of one training step (PlanFusedStep items of any kind): one multi launch per optimizer kind.  A net with only
    SGD optimizers makes the one Matrix.SGDMomentumStepMulti call it always made."""
    by_kind = {}
    for it in items:
        by_kind.setdefault(type(it), []).append(it)
    for kind, group in by_kind.items():
        kind.multi(group)


class SGDOptimizer(Optimizer):
    def __init__(self, c):
        super().__init__(c)
        self.gradient_clip_ = c.gradient_clip
        self.initial_momentum_ = c.initial_momentum
        self.final_momentum_ = c.final_momentum
        self.momentum_transition_timescale_ = c.momentum_transition_timescale
        self.nesterov_momentum_ = c.nesterov_momentum
        self.gradient_history_ = Matrix()
        self.fused = False

    def AllocateMemory(self, rows, cols, storage=None, storage2=None):
        """``storage``: optional Matrix slice of a flat history buffer (the reference allocates one
        matrix per tensor, src/optimizer.cc:131-134; a flat buffer makes the state contiguous).  ``storage2``: the same for the
        second-moment history of the subclasses that keep one."""
        if storage is not None:
            self.gradient_history_ = storage
            self.gradient_history_.Reshape(rows, cols)
        else:
            self.gradient_history_.AllocateGPUMemory(rows, cols, "optimizer")
        self.gradient_history_.Set(0.0)

    def IsAllocated(self):
        return self.gradient_history_.GetNumEls() > 0

    def LoadParameters(self, file, prefix):
        # src/optimizer.cc:138-146
        self.gradient_history_.ReadHDF5(file, f"{prefix}_gradient_history")
        self.step_ = file.ReadHDF5IntAttr(f"{prefix}_step", self.step_)

    def SaveParameters(self, file, prefix):
        # src/optimizer.cc:148-156
        self.gradient_history_.WriteHDF5(file, f"{prefix}_gradient_history")
        file.WriteHDF5IntAttr(f"{prefix}_step", self.step_)

    def GetMomentum(self):
        # src/optimizer.cc:158-165 in float, like the reference (expf of a float argument)
        f32 = np.float32
        if self.momentum_transition_timescale_ > 0:
            x = f32(-f32(self.step_) / f32(self.momentum_transition_timescale_))
            return float(f32(f32(self.initial_momentum_) + f32(f32(f32(self.final_momentum_) - f32(self.initial_momentum_)) * f32(f32(1) - _expf(x)))))
        return self.final_momentum_

    def NotifyStart(self, parameter):
        if self.nesterov_momentum_:
            self.gradient_history_.Mult(self.GetMomentum())
            parameter.Add(self.gradient_history_, -1)

    def PlanFusedStep(self, gradient, parameter):
        """The plain fused step of Optimize as DATA — an SGDStep (gradient, parameter, history, l2, clip, epsilon, momentum) for
        Matrix.SGDMomentumStepMulti, or the subclass's kind, for RunFusedSteps — with the step counter advanced exactly as Optimize would;
        None when this optimizer's step is not the plain one (unfused host, Nesterov, a norm limit / constraint, still before start_optimization_after): the caller runs Optimize."""
        if (not self.fused or self.nesterov_momentum_ or self.weight_norm_constraint_ > 0 or self.weight_norm_limit_ > 0 or
                self.step_ < self.start_optimization_after_):
            return None
        item = self._fused_item(gradient, parameter)
        self.step_ += 1
        return item

    def _fused_item(self, gradient, parameter):
        """This optimizer kind's plain fused step at the current step count: the subclasses' part of PlanFusedStep."""
        return SGDStep(gradient, parameter, self.gradient_history_, self.l2_decay_, self.gradient_clip_, self.GetDecayedEpsilon(), self.GetMomentum())

    def Optimize(self, gradient, parameter):
        # src/optimizer.cc:174-200
        if self.step_ >= self.start_optimization_after_:
            epsilon = self.GetDecayedEpsilon()
            if self.fused and not self.nesterov_momentum_:
                if self.weight_norm_constraint_ > 0 or self.weight_norm_limit_ > 0:
                    con = self.weight_norm_constraint_ > 0
                    Matrix.SGDMomentumStepNormLimit(gradient, parameter, self.gradient_history_, self.l2_decay_, self.gradient_clip_,
                                                    epsilon, self.GetMomentum(),
                                                    self.weight_norm_constraint_ if con else self.weight_norm_limit_, con)
                else:
                    Matrix.SGDMomentumStep(gradient, parameter, self.gradient_history_, self.l2_decay_,
                                           self.gradient_clip_, epsilon, self.GetMomentum())
                self.step_ += 1
                return
            else:
                if self.l2_decay_ > 0:
                    gradient.Add(parameter, self.l2_decay_)
                if self.gradient_clip_ > 0:
                    gradient.UpperBoundMod(self.gradient_clip_)
                gradient.Mult(epsilon)
                if not self.nesterov_momentum_:
                    self.gradient_history_.Mult(self.GetMomentum())
                self.gradient_history_.Add(gradient)
                if self.nesterov_momentum_:
                    parameter.Add(gradient, -1)
                else:
                    parameter.Add(self.gradient_history_, -1)
            self.ApplyConstraints(parameter)
        self.step_ += 1


class _SecondMomentSGDOptimizer(SGDOptimizer):
    """What AdagradSGDOptimizer and RMSPropSGDOptimizer share (src/optimizer.cc:202-255): a second history beside the momentum one, with
    its initial value and its dataset name in a checkpoint."""
    history_name_ = None

    def __init__(self, c, initial):
        super().__init__(c)
        self.second_history_ = Matrix()
        self.second_history_initial_ = initial

    def NeedsSecondHistory(self):
        return True

    def AllocateMemory(self, rows, cols, storage=None, storage2=None):
        super().AllocateMemory(rows, cols, storage)
        if storage2 is not None:
            self.second_history_ = storage2
            self.second_history_.Reshape(rows, cols)
        else:
            self.second_history_.AllocateGPUMemory(rows, cols, "optimizer")
        self.second_history_.Set(self.second_history_initial_)

    def IsAllocated(self):
        return self.second_history_.GetNumEls() > 0

    def LoadParameters(self, file, prefix):
        super().LoadParameters(file, prefix)
        self.second_history_.ReadHDF5(file, f"{prefix}_{self.history_name_}")

    def SaveParameters(self, file, prefix):
        # The reference writes gradient_history_ a second time under this name (src/optimizer.cc:219-224, 250-255) and reads the
        # dataset back into the second-moment history: its own checkpoints do not resume.  Here the dataset holds what is read back.
        super().SaveParameters(file, prefix)
        self.second_history_.WriteHDF5(file, f"{prefix}_{self.history_name_}")

    def _fuses_now(self):
        return self.fused and not self.nesterov_momentum_ and self.step_ >= self.start_optimization_after_

    def _run_fused(self, gradient, parameter):
        item = self._fused_item(gradient, parameter)
        item.multi([item])
        self.ApplyConstraints(parameter)
        self.step_ += 1


class AdagradSGDOptimizer(_SecondMomentSGDOptimizer):
    history_name_ = "adagrad_history"

    def __init__(self, c):
        super().__init__(c, c.adagrad_delta)      # src/optimizer.cc:206-210: the history starts at delta
        self.adagrad_delta_ = c.adagrad_delta

    adagrad_history_ = property(lambda self: self.second_history_)

    def _step_scale(self):
        return float(np.float32(math.sqrt(self.step_ + 1)))   # sqrt(int) is the double one; Mult(float) rounds it once

    def _fused_item(self, gradient, parameter):
        return AdagradStep(gradient, parameter, self.gradient_history_, self.second_history_, self.adagrad_delta_, self._step_scale(),
                           self.l2_decay_, self.gradient_clip_, self.GetDecayedEpsilon(), self.GetMomentum())

    def Optimize(self, gradient, parameter):
        # src/optimizer.cc:226-231.  The history update and the rescaling run on every call, also before start_optimization_after.
        if self._fuses_now():
            self._run_fused(gradient, parameter)
            return
        h = self.second_history_
        h.AdagradUpdate(h, gradient, self.adagrad_delta_)      # Matrix::AdagradUpdate, a static of the history's class
        gradient.Divide(self.second_history_)
        gradient.Mult(self._step_scale())
        super().Optimize(gradient, parameter)       # Nesterov, the unfused host or before the start: the reference's sequence there too


class RMSPropSGDOptimizer(_SecondMomentSGDOptimizer):
    history_name_ = "rms_history"

    def __init__(self, c):
        super().__init__(c, 1.0)                  # src/optimizer.cc:237-241
        self.factor_ = c.rms_prop_factor

    rms_history_ = property(lambda self: self.second_history_)

    def _fused_item(self, gradient, parameter):
        return RMSPropStep(gradient, parameter, self.gradient_history_, self.second_history_, self.factor_, self.l2_decay_, self.gradient_clip_,
                           self.GetDecayedEpsilon(), self.GetMomentum())

    def Optimize(self, gradient, parameter):
        # src/optimizer.cc:257-279.  nesterov_momentum plays no part in here (the inherited NotifyStart still acts on it).
        if self._fuses_now():
            self._run_fused(gradient, parameter)
            return
        if self.step_ >= self.start_optimization_after_:
            epsilon, momentum = self.GetDecayedEpsilon(), self.GetMomentum()
            self.gradient_history_.Mult(momentum)
            if self.l2_decay_ > 0:
                gradient.Add(parameter, self.l2_decay_)
            if self.gradient_clip_ > 0:
                gradient.UpperBoundMod(self.gradient_clip_)
            h = self.second_history_
            h.RMSPropUpdate(h, gradient, self.factor_)             # Matrix::RMSPropUpdate, a static of the history's class
            gradient.Divide(self.second_history_)
            self.gradient_history_.Add(gradient, epsilon)
            parameter.Add(self.gradient_history_, -1)
            self.ApplyConstraints(parameter)
        self.step_ += 1
