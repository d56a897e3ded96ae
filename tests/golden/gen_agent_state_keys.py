"""Writes tests/golden/agent_state_keys.json: for each agent of armenv.checkpoint and the state widths 6 (reach) and 9 (push, pick),
the files that the reference's ``agent.save(filename)`` writes and, per file, the ``state_dict()`` keys and shapes of the module it
saves -- names and shapes only, read off the reference's own ``net_mlp`` modules at generation time (hidden 256, action_dim 3).

    python tests/golden/gen_agent_state_keys.py <path to the reference checkout>

The fixture is what tests/test_checkpoint_host.py holds ``save_agent``'s files against; the tests never import the reference."""
import importlib.util
import json
import os
import sys

# agent -> (the reference's algo directory, [(suffix, class of net_mlp)]) in the order of its save()
AGENTS = dict(td3=("TD3", [("_critic.pt", "QValueNet"), ("_actor.pt", "PolicyNet")]),
              daddpg=("DADDPG", [("_critic.pt", "QValueNet"), ("_actor1.pt", "PolicyNet"), ("_actor2.pt", "PolicyNet")]),
              datd3=("DATD3", [("_critic1.pt", "QValueNet"), ("_actor1.pt", "PolicyNet"), ("_critic2.pt", "QValueNet"), ("_actor2.pt", "PolicyNet")]),
              darc=("DARC", [("_critic1.pt", "QValueNet"), ("_actor1.pt", "PolicyNet"), ("_critic2.pt", "QValueNet"), ("_actor2.pt", "PolicyNet")]))


def _net_mlp(reference, algo):
    spec = importlib.util.spec_from_file_location("ref_%s_net_mlp" % algo, os.path.join(reference, "algo", algo, "net_mlp.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def main(reference):
    out = {}
    for state_dim in (6, 9):
        per_agent = {}
        for agent, (algo, files) in AGENTS.items():
            nets = _net_mlp(reference, algo)
            per_agent[agent] = {}
            for suffix, cls in files:
                net = nets.PolicyNet(state_dim, 256, 3, 1.0) if cls == "PolicyNet" else nets.QValueNet(state_dim, 256, 3)
                per_agent[agent][suffix] = [[k, list(v.shape)] for k, v in net.state_dict().items()]
                assert all(str(v.dtype) == "torch.float32" for v in net.state_dict().values())
        out[str(state_dim)] = per_agent
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "agent_state_keys.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(path)


if __name__ == "__main__":
    main(sys.argv[1])
