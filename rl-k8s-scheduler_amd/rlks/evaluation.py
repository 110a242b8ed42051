"""Batched evaluation harness: the reference's evaluation and baseline loops, one env lane per episode.

Reference loops restated here (all sequential over ONE env and the process-global `random` stream):
  * final_evaluation.py:39-77 — 100 greedy episodes (`compute_single_action(obs, explore=False)`),
    per-episode cost `-ep_reward`, AWS / Azure choice counts, improvement vs the 4.765 greedy
    baseline, summary text (:80-82);
  * train_and_compare.py:53-79 — the round-robin baseline (`0 if env.current_step % 2 == 0 else 1`)
    and the side-by-side RL vs baseline table;
  * k8s_multi_cloud_env.py:156-157 — the cost-only greedy scheduler `normal_scheduler_step`.

Here episode e runs on lane e of a VecK8sMultiCloudEnv in CPython-MT19937 mode, and every lane
steps in the same kernel launch.  Lane e's generator is seeded like `random.seed(seed)` and then
advanced (rlks_env_mt_discard) by the 200 random() draws each earlier episode consumes (2 per
observation: reset + 99 steps), so lane e sees exactly the cpu-load draws episode e of the
reference's sequential loop sees.  Episode returns accumulate in float64 in step order from 0.0,
as `ep_reward += reward` does, so rewards, choices and costs equal the sequential loop's bit for bit
(tests/test_gpu_eval.py checks this against the drop-in env driven step by step).

Baselines beyond the reference's two, and node-level envs: the rule names of
rlks._lib.RULES are decided on the device by rlks_env_rule_actions, one launch ahead of the step, so a
baseline's loop is as device-resident as a policy's.  evaluate_nodes() is the harness for node-level
envs (returns, choices, placed / rejected / departed pods, utilisation); comparison_report() prints
policies and baselines side by side, as train_and_compare.py:75-79 and final_evaluation.py:73-74 do.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .env import VecK8sMultiCloudEnv
from .sampling import mask_on, resolve_policy
from .tables import load_table

BASELINE_COST = 4.765          # final_evaluation.py:73
DRAWS_PER_OBS = 2              # _get_obs: cpu_aws, cpu_azure (k8s_multi_cloud_env.py:92-93)
CLOUD_NAMES = ("AWS", "Azure")  # action 0 / 1 (final_evaluation.py:51)


@dataclass
class EvalResult:
    rewards: np.ndarray                 # float64 [episodes], sum of step rewards
    actions: np.ndarray                 # int32 [steps, episodes]
    baseline_cost: float = BASELINE_COST
    names: tuple = CLOUD_NAMES
    extra: dict = field(default_factory=dict)

    @property
    def costs(self) -> np.ndarray:      # final_evaluation.py:60
        return -self.rewards

    @property
    def avg_cost(self) -> float:        # :62
        return float(np.mean(self.costs))

    @property
    def choices(self) -> dict:          # :40, :51
        counts = np.bincount(self.actions.reshape(-1), minlength=len(self.names))
        return {n: int(c) for n, c in zip(self.names, counts)}

    @property
    def improvement(self) -> float:     # :74
        return 100 * (self.baseline_cost - self.avg_cost) / self.baseline_cost

    def progress_lines(self, every=20):
        """the per-episode progress prints of :54-55"""
        return [f"Episode {ep:3d} → cost = ${-self.rewards[ep - 1]:6.3f}"
                for ep in range(every, len(self.rewards) + 1, every)]

    def report(self) -> str:
        """the results block of final_evaluation.py:64-77"""
        ch = self.choices
        total = sum(ch.values())
        lines = ["", "=" * 60, f"FINAL EVALUATION RESULTS ({len(self.rewards)} episodes)", "=" * 60,
                 f"Average cost per episode       : ${self.avg_cost:.4f}",
                 f"Total decisions total           : {total}"]
        for n in self.names:
            lines.append(f"Agent chose {n:<19}: {ch[n]:4d} times ({ch[n] / total:.1%})")
        lines += ["", f"Improvement vs greedy baseline (${self.baseline_cost:.3f}): {self.improvement:5.1f}% better",
                  "=" * 60]
        return "\n".join(lines)

    def summary_text(self) -> str:
        """the summary file body of :80-82"""
        ch = self.choices
        return (f"Avg cost: ${self.avg_cost:.4f} | Improvement: {self.improvement:.1f}%\n"
                f"{self.names[0]} choices: {ch[self.names[0]]} | {self.names[1]} choices: {ch[self.names[1]]}\n")


def decider(policy, env, *, explore=False, masked=False, table_rules=False):
    """The decide step of every loop here and of DecisionLog.collect, built once per run -> (decide, forward):
    decide(obs, t) -> (actions int32 [N], logp float32 [N] or None) for `env`'s lanes.  `policy`: a
    sampling.Policy, which decides by forward(obs) (the logits, in scratch owned here; None for a rule) and then
    their first maximum (np.argmax) or, with `masked`, env.masked_sample(logits, explore=explore); or a rule
    name, decided on the device by env.rule_actions -- except that with `table_rules` "round_robin" and "greedy"
    are the reference's two table-env baselines (train_and_compare.py:65, k8s_multi_cloud_env.py:156-157)."""
    import torch

    N, dev = env.num_envs, env.device
    if isinstance(policy, str):
        if table_rules and policy == "round_robin":
            return (lambda obs, t: (torch.full((N,), t % 2, dtype=torch.int32, device=dev), None)), None
        if table_rules and policy == "greedy":
            return (lambda obs, t: ((obs[:, 0] > obs[:, 1]).to(torch.int32), None)), None
        return (lambda obs, t: (env.rule_actions(policy), None)), None
    logits = torch.empty(N, env.n_clouds, dtype=torch.float32, device=dev)
    values = torch.empty(N, dtype=torch.float32, device=dev)

    def forward(obs):
        if policy.filter is not None:
            obs = policy.filter.apply(obs)
        return policy.params.forward(obs, logits, values)[0]

    if masked:
        return (lambda obs, t: env.masked_sample(forward(obs), explore=explore)), forward
    return (lambda obs, t: (torch.argmax(forward(obs), dim=1).to(torch.int32), None)), forward


def run_episodes(env, obs, decide, steps, *, actions=False, util=False, check_done=True):
    """`steps` steps of a prepared env (seeded and reset by the caller: obs is what reset() returned) under
    `decide`.  -> (returns float64 [N], summed in step order from 0.0 as `ep_reward += reward` does; the
    actions int32 [steps, N] or None; the utilisation columns of every step's observation summed, float64
    [N, C], or None): device tensors.  Raises what check_status raises, and RuntimeError when check_done and
    a lane has not terminated."""
    import torch

    N, C_ = env.num_envs, env.n_clouds
    ret = torch.zeros(N, dtype=torch.float64, device=env.device)
    acts = torch.empty(steps, N, dtype=torch.int32, device=env.device) if actions else None
    usum = torch.zeros(N, C_, dtype=torch.float64, device=env.device) if util else None
    for t in range(steps):
        a = decide(obs, t)[0]
        if acts is not None:
            acts[t] = a
        obs, r, term, _, _ = env.step(a)
        ret += r
        if usum is not None:
            usum += obs[:, 2 * C_:]
    env.check_status()
    if check_done and not bool(term.all()):
        raise RuntimeError("evaluation lanes did not terminate after max_steps")
    return ret, acts, usum


def evaluate(policy, num_episodes: int = 100, *, seed=None, table=None, device=None,
             baseline_cost: float = BASELINE_COST) -> EvalResult:
    """final_evaluation.py:39-77 batched: `policy` is a PPO algorithm / PolicyParams (greedy argmax,
    compute_single_action(obs, explore=False)), or "round_robin" / "greedy" for the baselines, or a
    device rule (VecK8sMultiCloudEnv.rule_actions): "cheapest" (= "greedy"), "myopic" (the largest
    immediate reward: the optimal policy of the table env, whose reward depends on nothing the agent
    changes), "least_loaded", "myopic_with_room" (= "myopic" here: a table env always has room) and
    "random" (Philox draws keyed by `seed`).

    seed: the value of the reference's `random.seed(seed)` before its first episode (its env is
    unseeded, so the process-global stream decides; None draws one from this process's `random`)."""
    import torch

    if num_episodes <= 0:
        raise ValueError("num_episodes must be positive")
    table = table if table is not None else load_table()
    if isinstance(policy, str):
        if policy not in ("round_robin", "greedy") and policy not in _lib.RULES:
            raise ValueError(f"unknown baseline policy {policy!r}")
    else:
        policy = resolve_policy(policy, table)
        device = policy.params.flat.device if device is None else device
    if seed is None:
        seed = random.getrandbits(64)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    E = int(num_episodes)
    T = table.n_rows - 1  # max_steps (:66): every episode is exactly 99 steps
    # (the env's own seed keys only the "random" rule's Philox draws: the MT19937 lanes are seeded below)
    env = VecK8sMultiCloudEnv(E, table=table, noise="mt19937", autoreset=False, device=device,
                              seed=int(seed) if policy == "random" else 0)
    try:
        env.seed([int(seed)] * E)
        per_episode = DRAWS_PER_OBS * (T + 1)
        skip = torch.arange(E, dtype=torch.int64, device=env.device) * per_episode
        _lib.call("rlks_env_mt_discard", env.handle, None, _lib.ptr(skip), env.dev.stream)
        ret, actions, _ = run_episodes(env, env.reset(), decider(policy, env, table_rules=True)[0], T, actions=True)
        return EvalResult(ret.cpu().numpy(), actions.cpu().numpy(), baseline_cost,
                          CLOUD_NAMES if table.n_clouds == 2 else tuple(f"cluster{c}" for c in range(table.n_clouds)),
                          {"seed": int(seed)})
    finally:
        env.close()


def _node_run(policy, num_episodes, table, nodes, seed, device, action_mask, full):
    """the run behind evaluate_nodes (`full`: with the actions, the utilisation sums and the env's counters,
    which cost atomics and change no result) and evaluate_lanes: lane e of a Philox env keyed by `seed` =
    episode e, autoreset off, max_steps steps.  -> run_episodes' triple and the counters on the host (or None)"""
    pol = None
    if not isinstance(policy, str):
        policy = pol = resolve_policy(policy, table)
        if device is None:
            device = pol.params.flat.device
    mask = mask_on(pol, action_mask, nodes)
    env = VecK8sMultiCloudEnv(int(num_episodes), table=table, seed=int(seed), noise="philox", autoreset=False,
                              device=device, nodes=nodes)
    try:
        if full:
            env.counters(enable=1)
        out = run_episodes(env, env.reset(), decider(policy, env, masked=mask)[0], env.max_steps, actions=full, util=full,
                           check_done=full)
        return (*out, env.counters().cpu().numpy() if full else None)
    finally:
        env.close()


def evaluate_lanes(params, num_episodes: int, *, table=None, nodes=None, seed=0, device=None,
                   action_mask=None) -> np.ndarray:
    """Greedy (explore=False) float64 returns of `num_episodes` episodes, one lane each, all lanes
    in one batched env: RLlib's evaluation workers (train_final.py:19 .evaluation(
    evaluation_interval=5, evaluation_duration=20), evaluation explore=False).  Table envs run the
    reference-exact evaluate() above; node-level envs (configs c3 / c5) run evaluate_nodes' loop without its
    counters, so the returns are evaluate_nodes(...).rewards.  action_mask (None = the setting of a PPO
    algorithm passed as `params`, off otherwise): decide with VecK8sMultiCloudEnv.masked_sample(logits,
    explore=False), the argmax over the clusters with room."""
    table = table if table is not None else load_table()
    if nodes is None:
        mask_on(resolve_policy(params), action_mask, None)  # asking for a mask here is an error
        return evaluate(params, num_episodes, seed=seed, table=table, device=device).rewards
    return _node_run(params, num_episodes, table, nodes, seed, device, action_mask, False)[0].cpu().numpy()


@dataclass
class NodeEvalResult:
    """evaluate_nodes(): one episode per lane of a node-level env"""
    rewards: np.ndarray      # float64 [episodes], step rewards summed in step order
    actions: np.ndarray      # int32 [steps, episodes]
    choices: np.ndarray      # int64 [C]: decisions per cluster (sums to steps * episodes)
    placed: int              # pods placed, rejected (no node of the chosen cluster had room), departed
    rejected: int
    departed: int
    mean_util: np.ndarray    # float64 [C]: mean cpu utilisation observed after each step, over steps and lanes
    extra: dict = field(default_factory=dict)

    @property
    def rejection_rate(self) -> float:
        """rejected / arrived pods (0 when none arrived)"""
        n = self.placed + self.rejected
        return self.rejected / n if n else 0.0


def evaluate_nodes(policy, num_episodes: int, *, nodes, table=None, seed=0, device=None,
                   action_mask=None) -> NodeEvalResult:
    """`num_episodes` episodes of a node-level env (rlks.env.NodeSpec `nodes`), one lane each, every lane
    stepped by the same launches: episode e runs on lane e of a Philox env keyed by `seed`, with
    autoreset=False, for max_steps steps.  `policy`: a PPO algorithm or PolicyParams (greedy argmax, as
    evaluate_lanes and RLlib's evaluation workers, explore=False) or a rule name of rlks._lib.RULES
    (decided on the device by rlks_env_rule_actions).  Returns are summed in float64 in step order,
    as evaluate_lanes sums them; the pod counts are rlks_env_counters'.  The loop stays on the device:
    everything is read back once at the end.  action_mask (None = the setting of a PPO algorithm passed
    as `policy`, off otherwise): the policy decides with masked_sample(logits, explore=False), the argmax
    over the clusters with room.

    The comparison of two policies is paired: arrivals are keyed by (lane, episode, step), not by what
    was decided, so two calls with the same `seed` and episode count see the same arrival counts at
    every step (placed + rejected is the same), and the same initial occupancy; only placements, and
    with them the departures, differ."""
    if num_episodes <= 0:
        raise ValueError("num_episodes must be positive")
    if nodes is None:
        raise ValueError("evaluate_nodes needs a NodeSpec; table envs are evaluate()'s")
    table = table if table is not None else load_table()
    if isinstance(policy, str) and policy not in _lib.RULES:
        raise ValueError(f"unknown baseline policy {policy!r}; one of {sorted(_lib.RULES)}")
    ret, actions, util, k = _node_run(policy, num_episodes, table, nodes, seed, device, action_mask, True)
    acts = actions.cpu().numpy()
    T, E = acts.shape
    return NodeEvalResult(ret.cpu().numpy(), acts, np.bincount(acts.reshape(-1), minlength=table.n_clouds).astype(np.int64),
                          int(k[1]), int(k[2]), int(k[3]), util.sum(0).cpu().numpy() / (T * E), {"seed": int(seed)})


def comparison_report(results: dict, baseline: str | None = None) -> str:
    """One line per policy of `results` (name -> EvalResult or NodeEvalResult): mean return,
    improvement over `baseline` (a key of results; default: the first) in percent of its mean return,
    rejection rate (node-level results) and the share of decisions each cluster got -- the "RL vs
    baseline" table of train_and_compare.py:75-79 and the "improvement vs the greedy baseline" of
    final_evaluation.py:73-74 for any number of policies."""
    if not results:
        raise ValueError("comparison_report needs at least one result")
    baseline = next(iter(results)) if baseline is None else baseline
    if baseline not in results:
        raise ValueError(f"baseline {baseline!r} is not among the results {list(results)}")
    base = float(np.mean(results[baseline].rewards))
    width = max(len(str(n)) for n in results)
    lines = []
    for name, res in results.items():
        mean = float(np.mean(res.rewards))
        ch = res.choices
        counts = np.array(list(ch.values()) if isinstance(ch, dict) else ch, np.float64)
        shares = " ".join(f"{x:.1%}" for x in counts / max(counts.sum(), 1.0))
        imp = 100.0 * (mean - base) / abs(base) if base else float("nan")
        rej = f"{res.rejection_rate:7.2%}" if hasattr(res, "rejection_rate") else "    n/a"
        lines.append(f"{str(name):<{width}} : return = {mean:10.2f} | vs {baseline} = {imp:+7.2f}% | "
                     f"rejected = {rej} | choices = {shares}")
    return "\n".join(lines)


def round_robin_baseline(num_episodes: int = 5, **kw) -> np.ndarray:
    """train_and_compare.py:53-72: per-episode round-robin returns"""
    return evaluate("round_robin", num_episodes, **kw).rewards


def comparison_lines(rl_rewards, baseline_rewards):
    """train_and_compare.py:75-79: the side-by-side table"""
    return [f"Iteration {i + 1}: RL = {r:.2f} | Baseline = {b:.2f}"
            for i, (r, b) in enumerate(zip(rl_rewards, baseline_rewards))]
