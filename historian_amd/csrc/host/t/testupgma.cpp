// testupgma <modelfile> <alignfile>: the tree of a gapped alignment's rows by UPGMA over the maximum-likelihood distance
// matrix, as Newick (the reference's t/testupgma.cpp).  The distances come from the device; HX_HOST_DISTANCES=1: from the host.
#include <iostream>
#include "../hx_host.h"
using namespace historian;

int main(int argc, char** argv) {
  if (argc != 3) {
    std::cout << "Usage: " << argv[0] << " <modelfile> <alignfile>\n";
    exit(EXIT_FAILURE);
  }
  RateModel rates;
  rates.readFile(argv[1]);
  const vguard<FastSeq> gapped = readFastSeqs(argv[2]);
  const auto dist = rates.distanceMatrix(gapped);
  vguard<string> names;
  for (const auto& fs : gapped) names.push_back(fs.name);
  ReconTree tree;
  tree.buildByUPGMA(names, dist);
  std::cout << tree.toString() << std::endl;
  exit(EXIT_SUCCESS);
}
