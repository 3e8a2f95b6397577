// nh_taxa.h -- the taxa manifest of nh_build_db (nh_build_args.taxa_file): host only, no device, no HIP.
//
//   taxid <TAB> parent taxid <TAB> name [<TAB> FASTA path]...
//
// one taxon a line; `#` lines and empty lines are skipped, CRLF is tolerated.  A line without a path is an inner node; a node with
// children may carry sequences too.  Parent 1 is the root, which is implicit and never a line.  Relative paths resolve against the
// manifest's directory.  Internal ids: 0 the null sentinel, 1 the root, then breadth first with the children of a node in ascending
// external id -- parents lie below their children, and the lowest common ancestor of two nodes is found by walking the larger id up.
#ifndef NH_TAXA_H
#define NH_TAXA_H
#include <stdint.h>

#include <string>
#include <vector>

namespace nh {

constexpr uint32_t TAXA_MAX_NODES = 4096;  // taxa and the root; with the sentinel 4097 values: value_bits <= 13

struct TaxaNode {
    uint64_t taxid = 0;              // external id
    uint32_t parent = 0;             // internal id of the parent (0 for the sentinel and the root)
    uint32_t first_child = 0, children = 0;
    uint32_t line = 0;               // of the manifest (0: the sentinel, the root)
    std::string name;
    std::vector<std::string> files;  // FASTA paths, resolved
};

// the manifest at `path` -> nodes in internal-id order ([0] the sentinel, [1] the root).  NH_OK, or NH_EINVAL / NH_EIO with a
// message that names the file and the line.
int parse_taxa(const char *path, std::vector<TaxaNode> &nodes, std::string &err);

// bits of a cell's value field for that many nodes, the sentinel included (2 for three nodes)
inline uint32_t value_bits_for(uint32_t node_count) {
    uint32_t b = 1;
    while ((1u << b) < node_count) b++;
    return b;
}

}  // namespace nh
#endif
