// <lib>.kmer.freq.stat -- the k-mer frequency spectrum as the original kmerfreq prints it next to its table (the
// reference ships three of them under test/01.clean_correct/).  One function, histogram to text; no GPU in it.
//
// Five '#' lines, an empty line, the column header, then one row per frequency 1..max_freq:
//   frequency, species, species / total species, accumulated, individuals, individuals / total individuals, accumulated
// Doubles go out through the stream's default formatting.  The accumulated columns are accumulated COUNTS divided
// by the total, so no sum of ratios is involved.  The last row's individual number is what the rows before it leave
// of total_individuals: for a histogram that is not cut off this equals freq * species; for saturating counters it
// makes the last row "max_freq or more" exact and every ratio column end at 1.  With no species or no individuals the
// ratios print 0 (the original would print nan).
#pragma once

#include <cstdint>
#include <ostream>

// species[f] = number of distinct k-mers seen f times, f = 1..max_freq (species[0] is not read)
inline void write_kmer_spectrum(std::ostream &out, int k, uint32_t max_freq, const uint64_t *species, uint64_t total_individuals)
{
	uint64_t total_species = 0;
	for (uint32_t f = 1; f <= max_freq; ++f) total_species += species[f];
	const uint64_t space = 1ull << (2 * k);
	auto ratio = [](uint64_t a, uint64_t b) { return b ? (double)a / (double)b : 0.0; };
	out << "#Kmer size: " << k << "\n"
	    << "#Maximum Kmer frequency: " << max_freq << "\n"
	    << "#Kmer indivdual number: " << total_individuals << "\n"
	    << "#Kmer species number: " << total_species << "\n"
	    << "#Theoretic space of Kmer species: " << space << "  occupied ratio: " << ratio(total_species, space) << "\n"
	    << "\n"
	    << "#Kmer_Frequency\tKmer_Species_Number\tKmer_Species_Ratio\tKmer_Species_accumulate_Ratio\tKmer_Individual_Number"
	    << "\tKmer_Individual_Ratio\tKmer_Individual_accumulate_ratio\n";
	uint64_t acc_species = 0, acc_individuals = 0;
	for (uint32_t f = 1; f <= max_freq; ++f) {
		const uint64_t left = total_individuals > acc_individuals ? total_individuals - acc_individuals : 0;
		const uint64_t individuals = f == max_freq ? left : (uint64_t)f * species[f];
		acc_species += species[f];
		acc_individuals += individuals;
		out << f << "\t" << species[f] << "\t" << ratio(species[f], total_species) << "\t" << ratio(acc_species, total_species) << "\t"
		    << individuals << "\t" << ratio(individuals, total_individuals) << "\t" << ratio(acc_individuals, total_individuals) << "\n";
	}
}
